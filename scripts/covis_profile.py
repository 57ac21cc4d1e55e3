"""GPU box: time of the covisibility update (ccm_covis_update) at the three sizes of ccm_slam_amd.sim3_correct.SIZES, median of interleaved repetitions
(device call, host evaluator, device call, ... on one box):
  call_us   ccm_covis_update host to host with a capacity that fits: checks, packing, one H2D copy, seven launches, one D2H copy, unpacking
  host_us   the same arguments through covis_math.h compiled for the host, on one thread (ccmh_covis_update_host)
  default_cap_us   the device call as cslam::CovisibilityBatch makes it, starting from its first guess max(4096, 96 n_kf) (the D2H copy is sized by the capacity;
            default_cap_calls says whether the guess had to grow), timed in a loop of its own after the interleaved one
Both go through the same ctypes binding, whose cost (array checks, output allocation) is in both figures.  Compare only rows of one run.
Prints one JSON line; --out FILE also writes it there.
Device time, in a run of its own: `rocprofv3 --kernel-trace --stats -d DIR -o cv -- python scripts/covis_profile.py --out A.json`, then
`python scripts/covis_profile.py --from-trace DIR/cv_results.db --runs A.json --out B.json --stats-csv C.csv`: the trace's launches are split by the call counts
each size recorded (seven launches per call); B.json is A.json with the median per call of the seven kernels' sum and of each kernel, C.csv the per-kernel summary."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import covis as V
from ccm_slam_amd._lib import Context

REPS = 15
WARM = 2
PER_CALL = ("count_kernel", "scan_rows_kernel", "count_kernel", "pair_kernel", "scan_final_kernel", "pair_kernel", "final_kernel")


def run(ctx, size):
    n_kf, n_pt = V.SIZES[size]
    sc = V.make_scene(seed=100 + n_kf, n_kf=n_kf, n_pt=n_pt)
    first = V.update(ctx, sc)                                     # finds the capacity; not timed
    cap = int(max(first["col"].size, first["fw_col"].size, first["ord_kf"].size))
    dev, host = [], []
    for i in range(WARM + REPS):
        t = time.perf_counter(); d = V.update(ctx, sc, cap=cap); a = time.perf_counter() - t
        t = time.perf_counter(); h = V.update_host(sc, cap=cap); b = time.perf_counter() - t
        assert d["calls"] == 1 and all(np.array_equal(d[k], h[k]) for k in ("col", "count", "fw_col", "fw_w", "ord_kf", "ord_w", "flags"))
        if i >= WARM:
            dev.append(a); host.append(b)
    dflt, n_dflt = [], 0
    for i in range(REPS):
        t = time.perf_counter(); d = V.update(ctx, sc); dflt.append(time.perf_counter() - t)
        n_dflt += d["calls"]
    call, hst = 1e6 * float(np.median(dev)), 1e6 * float(np.median(host))
    return dict(size=size, keyframes=n_kf, keyframes_all=int(sc["n_all"]), list_entries=int(sc["list_pt"].size), observations=int(sc["obs_kf"].size),
                row_entries=int(first["col"].size), cap=cap, call_us=round(call, 1), host_us=round(hst, 1), host_over_call=round(hst / call, 2),
                default_cap=max(4096, 96 * n_kf), default_cap_us=round(1e6 * float(np.median(dflt)), 1), default_cap_calls=n_dflt // REPS,
                host_over_default_cap=round(hst / (1e6 * float(np.median(dflt))), 2), calls=dict(untimed=first["calls"] + WARM, timed=REPS, after=n_dflt))


def from_trace(db_path, runs_path, out_path, csv_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = [(n, d) for n, d in db.execute("select name, duration from kernels order by start") if "covis_" in n]
    res = json.load(open(runs_path))
    n_call = len(PER_CALL)
    if len(rows) % n_call or any(PER_CALL[k % n_call] not in rows[k][0] for k in range(len(rows))):
        raise SystemExit("the trace's covis launches are not whole calls of seven")
    calls = [rows[k:k + n_call] for k in range(0, len(rows), n_call)]
    med = lambda v: round(float(np.median(v)) / 1e3, 1)
    o = 0
    for r in res["runs"]:
        o += r["calls"]["untimed"]
        mine = calls[o:o + r["calls"]["timed"]]; o += r["calls"]["timed"]
        r["kernels_us"] = med([sum(d for _, d in c) for c in mine])
        r["count_kernels_us"] = med([c[0][1] + c[2][1] for c in mine])
        r["pair_kernels_us"] = med([c[3][1] + c[5][1] for c in mine])
        r["scan_kernels_us"] = med([c[1][1] + c[4][1] for c in mine])
        r["final_kernel_us"] = med([c[6][1] for c in mine])
        o += r["calls"]["after"]
    if o > len(calls):
        raise SystemExit(f"trace holds {len(calls)} calls, the runs recorded {o}")
    res["kernel_source"] = "rocprofv3 --kernel-trace of the same script, medians per size (scripts/covis_profile.py --from-trace)"
    line = json.dumps(res)
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    if csv_path:
        by = {}
        for n, d in rows:
            by.setdefault(n, []).append(d)
        tot = sum(sum(v) for v in by.values())
        with open(csv_path, "w") as f:
            f.write('"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n')
            for n, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
                v = np.array(v, float)
                f.write('"%s",%d,%d,%f,%.2f,%d,%d,%f\n' % (n, len(v), v.sum(), v.mean(), 100 * v.sum() / tot, v.min(), v.max(), v.std()))


def main():
    if "--from-trace" in sys.argv:
        arg = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
        from_trace(arg("--from-trace"), arg("--runs"), arg("--out"), arg("--stats-csv"))
        return
    ctx = Context(0)
    runs = [run(ctx, s) for s in ("loop", "agent", "agents4")]
    ctx.close()
    line = json.dumps(dict(reps=REPS, runs=runs))
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
