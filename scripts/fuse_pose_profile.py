"""GPU box: host-to-host time of ccm_fuse_pose_eval against two baselines, per row (about 1 000 features per keyframe, points from fuse_pose.make_scene):
  agent           25 calls x 1 000 points + 1 x  8 000     an agent's keyframe
  server_merged  100 calls x 1 000 points + 1 x 25 000     a server keyframe in a merged map
  small            5 calls x   300 points + 1 x  1 000
    device_us      ccm_fuse_pose_eval, host to host through the Python wrapper
    host_1_us      the same arguments through fuse_math.h compiled for the host, one thread: BASELINE A
    fusebatch_us   the route of cslam::FuseBatch for the same answers: per direction one batch (host window search, one ccm_hamming_csr_multi launch) and the resolve
                   of every call: BASELINE B.  The projections (valid, u, v, level) that FuseBatch takes as inputs are computed BEFORE the clock starts, so this
                   column leaves out the host projection of that route and is a lower bound of it.
Each figure is the median of 15 repetitions; the candidates of a row are interleaved within every repetition.  The whole table is measured three times (`runs`);
margin_us = max - min of a baseline's three medians is what counts as a difference against that baseline.  Compare only figures of one invocation.
Per row also, from the host evaluator: the mean and the largest number of candidates per window and the share of pairs per status.  Prints one JSON line; --out FILE
also writes it there (profiles/fuse_pose_profile.json).

Device time and the call's parts:
  `CCM_DBG=fuse python scripts/fuse_pose_profile.py --device-only 2> DIR/phases.txt` (profiler off),
  `rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -o fp -- python scripts/fuse_pose_profile.py --device-only`, then
  `python scripts/fuse_pose_profile.py --from-trace DIR/fp_results.db --phases DIR/phases.txt --out profiles/fuse_pose_profile_traced.json`:
the medians per row of the kernel and of the two copies (from the trace) and of the library's three host phases (packing, upload + kernel + download, unpacking;
printed by the library under CCM_DBG=fuse in the run without the profiler).  Kernels and phases are split by the call counts of the --device-only mode (3 warm-up +
15 timed calls per row, in the order above), the copies are assigned to their row by the byte counts the library prints."""
import ctypes as C
import json
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import fuse_pose as fp
from ccm_slam_amd._lib import Context, _p, host

REPS = 15
WARM = 3
SIZES = list(fp.PROFILE_SIZES)


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
    got = fp.fuse_pose_eval_host(sc, want_cand=True)
    st = fp.unpack_table(got["table"])["status"]
    win = got["n_cand"][st >= 4]
    share = np.bincount(st.ravel(), minlength=8) / st.size
    return dict(pairs=int(st.size), features=int(sc.feat_off[-1]), cand_mean=round(float(win.mean()), 2) if win.size else 0.0, cand_max=int(win.max()) if win.size else 0,
                status_share={fp.STATUS[i]: round(float(share[i]), 4) for i in range(8)})


class FuseBatchRoute:
    """cslam::FuseBatch for the jobs of a scene: the first direction as one batch of C targets, the second as one batch of one target.  The projections it takes as
    inputs come from the host evaluator, once, before anything is timed."""

    def __init__(self, sc):
        h = self.h = host()
        h.ccmh_fuse_batch_create.restype = C.c_void_p
        h.ccmh_fuse_batch_create.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 14 + [C.c_float]
        h.ccmh_fuse_batch_resolve.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        h.ccmh_fuse_batch_destroy.argtypes = [C.c_void_p]; h.ccmh_fuse_batch_destroy.restype = None
        got = fp.fuse_pose_eval_host(sc, want_uv=True)
        t = fp.unpack_table(got["table"])
        self.sc = sc
        self.passes = []
        jobs = sc.jobs
        for group in (list(range(len(jobs) - 1)), [len(jobs) - 1]):
            kf_off = [0]; pt_off = [0]; kx = []; ky = []; oc = []; kd = []; va = []; u = []; v = []; lv = []; pd = []
            for j in group:
                k, p0, n = jobs[j]
                a, b = int(sc.feat_off[k]), int(sc.feat_off[k + 1])
                xy = sc.feat_xy[2 * a:2 * b].reshape(-1, 2)
                kx.append(xy[:, 0]); ky.append(xy[:, 1]); oc.append(sc.feat_octave[a:b].astype(np.int32)); kd.append(sc.feat_desc[32 * a:32 * b])
                o0, o1 = int(got["job_off"][j]), int(got["job_off"][j + 1])
                va.append((t["status"][o0:o1] >= 4).astype(np.uint8)); u.append(got["uv"][o0:o1, 0]); v.append(got["uv"][o0:o1, 1]); lv.append(t["level"][o0:o1])
                pd.append(sc.pt_desc[32 * p0:32 * (p0 + n)])
                kf_off.append(kf_off[-1] + b - a); pt_off.append(pt_off[-1] + n)
            cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs).astype(dt))
            self.passes.append(dict(S=len(group), KO=np.array(kf_off, np.int32), KX=cat(kx, np.float32), KY=cat(ky, np.float32), OC=cat(oc, np.int32), KD=cat(kd, np.uint8),
                                    B=np.ascontiguousarray(np.tile(np.array(fp.BOUNDS, np.float32), (len(group), 1))), PO=np.array(pt_off, np.int32), VA=cat(va, np.uint8),
                                    U=cat(u, np.float32), V=cat(v, np.float32), LV=cat(lv, np.int32), PD=cat(pd, np.uint8), n=[jobs[j][2] for j in group]))
        self.hits = None

    def run(self):
        sc = self.sc; h = self.h
        hits = []
        for p in self.passes:
            b = h.ccmh_fuse_batch_create(0, p["S"], _p(p["KO"]), _p(p["KX"]), _p(p["KY"]), _p(p["OC"]), _p(p["KD"]), _p(p["B"]), _p(sc.scale_factors), _p(sc.inv_sigma2),
                                         _p(p["PO"]), _p(p["VA"]), _p(p["U"]), _p(p["V"]), _p(p["LV"]), _p(p["PD"]), C.c_float(sc.th))
            if not b:
                raise RuntimeError("ccmh_fuse_batch_create failed")
            for s in range(p["S"]):
                n = p["n"][s]
                bi = np.zeros(n, np.int32); bd = np.zeros(n, np.int32)
                hits.append(h.ccmh_fuse_batch_resolve(b, s, None, n, _p(bi), _p(bd)))
            h.ccmh_fuse_batch_destroy(b)
        self.hits = hits


def one_run(ctx, scenes, routes):
    rows = []
    for name in SIZES:
        sc = scenes[name]
        fns = dict(device_us=lambda: fp.fuse_pose_eval(ctx, sc), host_1_us=lambda: fp.fuse_pose_eval_host(sc))
        if routes.get(name) is not None:
            fns["fusebatch_us"] = routes[name].run
        r = _interleaved(fns)
        c, p1, p2 = fp.PROFILE_SIZES[name]
        rows.append(dict(size=name, calls=c, P1=p1, P2=p2, baselines=["host_1_us"] + (["fusebatch_us"] if "fusebatch_us" in r else []), **r))
    return rows


def device_only():
    ctx = Context(0)
    for name in SIZES:
        sc = fp.profile_scene(name)
        for _ in range(WARM + REPS):
            fp.fuse_pose_eval(ctx, sc)
    ctx.close()


def from_trace(db_path, phases_path, out_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    per = WARM + REPS
    med = lambda v: round(float(np.median(v)) / 1e3, 1)
    kern = [d for n, d in db.execute("select name, duration from kernels order by start") if "fuse_pose_kernel" in n]
    if len(kern) != per * len(SIZES):
        raise SystemExit(f"trace holds {len(kern)} launches of fuse_pose_kernel, expected {per * len(SIZES)}")
    # the copies: whichever table or view of the trace holds them (its name differs between rocprofv3 releases), as (bytes, duration).  A call makes one H2D and
    # one D2H copy; they are told apart and assigned to their row by their sizes, which the library prints (a small download may not appear in the trace at all)
    copies = None
    for (name,) in db.execute("select name from sqlite_master where type in ('table', 'view') and lower(name) like '%memory_cop%'"):
        cols = [c[1] for c in db.execute(f"pragma table_info('{name}')")]
        if "start" in cols and "size" in cols and ("duration" in cols or "end" in cols):
            dur = "duration" if "duration" in cols else "(\"end\" - start)"
            copies = [(int(r[0]), r[1]) for r in db.execute(f"select size, {dur} from '{name}' order by start")]
            break
    phases = None
    if phases_path and os.path.exists(phases_path):
        pat = re.compile(r"\[fuse_pose\] K=(\d+) P=(\d+) J=(\d+) pairs=(\d+) pack_us=([\d.]+) device_us=([\d.]+) unpack_us=([\d.]+) up_bytes=(\d+) down_bytes=(\d+)")
        phases = [tuple(float(x) for x in m.groups()) for m in map(pat.search, open(phases_path)) if m]
        if len(phases) != per * len(SIZES):
            phases = None
    out = []
    for i, name in enumerate(SIZES):
        s = slice(i * per + WARM, (i + 1) * per)
        row = dict(size=name, kernel_us=med(kern[s]))
        if phases is not None:
            p = np.array(phases[s])
            row.update(pack_us=round(float(np.median(p[:, 4])), 1), device_phase_us=round(float(np.median(p[:, 5])), 1), unpack_us=round(float(np.median(p[:, 6])), 1),
                       up_bytes=int(p[0, 7]), down_bytes=int(p[0, 8]))
            total = row["pack_us"] + row["device_phase_us"] + row["unpack_us"]
            row["share"] = {k: round(row[k] / total, 3) for k in ("pack_us", "device_phase_us", "unpack_us")}
            row["share"]["kernel_us"] = round(row["kernel_us"] / total, 3)
            for key, nbytes in (("h2d_us", row["up_bytes"]), ("d2h_us", row["down_bytes"])):
                mine = [d for b, d in (copies or []) if b == nbytes]
                if len(mine) == per:
                    row[key] = med(mine[WARM:])
                    row["share"][key] = round(row[key] / total, 3)
                else:
                    row[key] = None
                    row.setdefault("copies", {})[key] = f"{len(mine)} copies of {nbytes} bytes in the trace, expected {per}"
        out.append(row)
    line = json.dumps(dict(kernel_source="rocprofv3 --kernel-trace --memory-copy-trace --stats of scripts/fuse_pose_profile.py --device-only, medians of 15; "
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
    scenes = {name: fp.profile_scene(name) for name in SIZES}
    about = {name: describe(sc) for name, sc in scenes.items()}
    routes = {}; notes = {}
    for name, sc in scenes.items():
        try:
            routes[name] = FuseBatchRoute(sc)
            routes[name].run()
            want = fp.fuse_pose_eval_host(sc)["n_hit"].tolist()
            if routes[name].hits != want:      # the same answers, or the column is not a baseline
                notes[name] = "fusebatch route: nFused differs from the host evaluator's in %d calls; not timed" % sum(a != b for a, b in zip(routes[name].hits, want))
                routes[name] = None
        except Exception as e:   # noqa: BLE001
            routes[name] = None
            notes[name] = f"fusebatch route not measured: {e!r}"
    runs = []
    for _ in range(3):
        ctx = Context(0)
        runs.append(one_run(ctx, scenes, routes))
        ctx.close()
    table = []
    for i, row in enumerate(runs[0]):
        keys = [k for k in row if k.endswith("_us")]
        margins = {"margin_vs_" + b: round(max(r[i][b] for r in runs) - min(r[i][b] for r in runs), 1) for b in row["baselines"]}
        table.append(dict({k: v for k, v in row.items() if not k.endswith("_us")}, **{k: [r[i][k] for r in runs] for k in keys}, **margins, **about[row["size"]],
                          **({"note": notes[row["size"]]} if row["size"] in notes else {})))
    line = json.dumps(dict(reps=REPS, runs=3, rows=table))
    print(line)
    if arg("--out"):
        with open(arg("--out"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
