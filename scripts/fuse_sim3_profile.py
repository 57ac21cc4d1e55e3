"""GPU box: host-to-host time of ccm_fuse_sim3_eval against the host evaluator, per size (keyframes x points, about 1 000 features per keyframe):
  loop             30 x 2 000     a loop closure
  merge_1_agent   500 x 3 000     MergeMaps with one agent's map
  merge_4_agents 1000 x 5 000     a four-agent merge
    device_us   ccm_fuse_sim3_eval, host to host through the Python wrapper
    host_1_us   the same arguments through fuse_math.h compiled for the host, one thread, as the reference runs SearchAndFuse: the BASELINE
Each figure is the median of 15 repetitions; the two candidates of a row are interleaved within every repetition.  The whole table is measured three times
(`runs`); margin_us = max - min of the baseline's three medians is what counts as a difference in that row.  Compare only figures of one invocation.
Per size also, from the host evaluator: the mean and the largest number of candidates per window (the size of vIndices over the pairs that reach the window)
and the share of pairs per status.  Prints one JSON line; --out FILE also writes it there (profiles/fuse_sim3_profile.json).

Device time and the call's parts:
  `CCM_DBG=fuse python scripts/fuse_sim3_profile.py --device-only 2> DIR/phases.txt` (profiler off),
  `rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -o fs -- python scripts/fuse_sim3_profile.py --device-only`, then
  `python scripts/fuse_sim3_profile.py --from-trace DIR/fs_results.db --phases DIR/phases.txt --out profiles/fuse_sim3_profile_traced.json`:
the medians per size of the kernel and of the two copies (from the trace) and of the library's three host phases (packing, upload + kernel + download, unpacking;
printed by the library under CCM_DBG=fuse in the run without the profiler), split by the call counts of the --device-only mode (3 warm-up + 15 timed calls per
size, in the order above)."""
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import fuse_sim3 as fs
from ccm_slam_amd._lib import Context

REPS = 15
WARM = 3
SIZES = list(fs.PROFILE_SIZES)


def _interleaved(fns):
    """medians (us) of the callables of `fns`, each called once per repetition, in turn"""
    for _ in range(WARM):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(REPS):
        for k, f in fns.items():
            t = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t)
    return {k: round(1e6 * float(np.median(v)), 1) for k, v in ts.items()}


def describe(sc):
    got = fs.fuse_sim3_eval_host(sc, want_cand=True)
    st = fs.unpack_table(got["table"])["status"]
    win = got["n_cand"][st >= 4]
    share = np.bincount(st.ravel(), minlength=8) / st.size
    return dict(pairs=int(st.size), features=int(sc.feat_off[-1]), cand_mean=round(float(win.mean()), 2) if win.size else 0.0, cand_max=int(win.max()) if win.size else 0,
                status_share={fs.STATUS[i]: round(float(share[i]), 4) for i in range(8)})


def one_run(ctx, scenes):
    rows = []
    for name in SIZES:
        sc = scenes[name]
        r = _interleaved(dict(device_us=lambda: fs.fuse_sim3_eval(ctx, sc), host_1_us=lambda: fs.fuse_sim3_eval_host(sc)))
        rows.append(dict(size=name, K=sc.K, P=sc.P, baseline="host_1_us", **r))
    return rows


def device_only():
    ctx = Context(0)
    for name in SIZES:
        sc = fs.profile_scene(name)
        for _ in range(WARM + REPS):
            fs.fuse_sim3_eval(ctx, sc)
    ctx.close()


def from_trace(db_path, phases_path, out_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    per = WARM + REPS
    med = lambda v: round(float(np.median(v)) / 1e3, 1)
    kern = [d for n, d in db.execute("select name, duration from kernels order by start") if "fuse_sim3_kernel" in n]
    if len(kern) != per * len(SIZES):
        raise SystemExit(f"trace holds {len(kern)} launches of fuse_sim3_kernel, expected {per * len(SIZES)}")
    # the copies: whichever table or view of the trace holds them (its name differs between rocprofv3 releases); each call makes one H2D and one D2H copy
    copies = None
    for (name,) in db.execute("select name from sqlite_master where type in ('table', 'view') and lower(name) like '%memory_cop%'"):
        cols = [c[1] for c in db.execute(f"pragma table_info('{name}')")]
        if "start" in cols and ("duration" in cols or "end" in cols):
            dur = "duration" if "duration" in cols else "(\"end\" - start)"
            rows = [r[0] for r in db.execute(f"select {dur} from '{name}' order by start")]
            if len(rows) >= 2 * per * len(SIZES):
                copies = rows[-2 * per * len(SIZES):]      # the context's own set-up copies, if any, come first
                break
    phases = None
    if phases_path and os.path.exists(phases_path):
        pat = re.compile(r"\[fuse\] K=(\d+) P=(\d+) pack_us=([\d.]+) device_us=([\d.]+) unpack_us=([\d.]+) up_bytes=(\d+) down_bytes=(\d+)")
        phases = [tuple(float(x) for x in m.groups()) for m in map(pat.search, open(phases_path)) if m]
        if len(phases) != per * len(SIZES):
            phases = None
    out = []
    for i, name in enumerate(SIZES):
        s = slice(i * per + WARM, (i + 1) * per)
        row = dict(size=name, kernel_us=med(kern[s]))
        if copies is not None:
            c = copies[2 * i * per:2 * (i + 1) * per]
            row.update(h2d_us=med(c[2 * WARM::2]), d2h_us=med(c[2 * WARM + 1::2]))
        else:
            row.update(h2d_us=None, d2h_us=None, copies="not in the trace")
        if phases is not None:
            p = np.array(phases[s])
            row.update(pack_us=round(float(np.median(p[:, 2])), 1), device_phase_us=round(float(np.median(p[:, 3])), 1), unpack_us=round(float(np.median(p[:, 4])), 1),
                       up_bytes=int(p[0, 5]), down_bytes=int(p[0, 6]))
            total = row["pack_us"] + row["device_phase_us"] + row["unpack_us"]
            row["share"] = {k: round(row[k] / total, 3) for k in ("pack_us", "device_phase_us", "unpack_us")}
            if row["d2h_us"] is not None:
                row["share"].update(kernel_us=round(row["kernel_us"] / total, 3), h2d_us=round(row["h2d_us"] / total, 3), d2h_us=round(row["d2h_us"] / total, 3))
        out.append(row)
    line = json.dumps(dict(kernel_source="rocprofv3 --kernel-trace --memory-copy-trace --stats of scripts/fuse_sim3_profile.py --device-only, medians of 15; "
                                         "host phases from the library's CCM_DBG=fuse lines of a --device-only run with the profiler off", rows=out))
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


def main():
    arg = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
    if "--device-only" in sys.argv:
        return device_only()
    if "--from-trace" in sys.argv:
        return from_trace(arg("--from-trace"), arg("--phases"), arg("--out"))
    scenes = {name: fs.profile_scene(name) for name in SIZES}
    about = {name: describe(sc) for name, sc in scenes.items()}
    runs = []
    for _ in range(3):
        ctx = Context(0)
        runs.append(one_run(ctx, scenes))
        ctx.close()
    table = []
    for i, row in enumerate(runs[0]):
        base = [r[i][row["baseline"]] for r in runs]
        keys = [k for k in row if k.endswith("_us")]
        table.append(dict({k: v for k, v in row.items() if not k.endswith("_us")}, **{k: [r[i][k] for r in runs] for k in keys},
                          margin_us=round(max(base) - min(base), 1), **about[row["size"]]))
    line = json.dumps(dict(reps=REPS, runs=3, rows=table))
    print(line)
    if arg("--out"):
        with open(arg("--out"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
