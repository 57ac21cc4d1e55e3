"""GPU box: time of the Sim3 map correction (ccm_sim3_correct_map) at the three sizes of ccm_slam_amd.sim3_correct.SIZES, median of interleaved repetitions
(device call, host evaluator, device call, ... on one box):
  call_us   ccm_sim3_correct_map host to host: packing, one H2D copy, two launches, one D2H copy, unpacking
  host_us   the same arguments through sim3_correct_math.h compiled for the host, on one thread (ccmh_sim3_correct_map_host)
Both go through the same ctypes binding, whose cost (array checks, output allocation) is in both figures.  Compare only rows of one run.
Prints one JSON line; --out FILE also writes it there.
Device time, in a run of its own: `rocprofv3 --kernel-trace --stats -d DIR -o s3c -- python scripts/sim3_correct_profile.py --out A.json`, then
`python scripts/sim3_correct_profile.py --from-trace DIR/s3c_results.db --runs A.json --out B.json --stats-csv C.csv`: the trace's two kernels are split by the
launch counts each size recorded; B.json is A.json with their medians added, C.csv the per-kernel summary."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import sim3_correct as S
from ccm_slam_amd._lib import Context

REPS = 15
WARM = 2


def run(ctx, size):
    n_kf, n_pt = S.SIZES[size]
    f = S.flatten_loop(S.make_scene(seed=100 + n_kf, n_kf=n_kf, n_pt=n_pt))
    dev, host = [], []
    for i in range(WARM + REPS):
        t = time.perf_counter(); S.correct_map(ctx, f); a = time.perf_counter() - t
        t = time.perf_counter(); S.correct_map_host(f); b = time.perf_counter() - t
        if i >= WARM:
            dev.append(a); host.append(b)
    call, hst = 1e6 * float(np.median(dev)), 1e6 * float(np.median(host))
    return dict(size=size, keyframes=n_kf, points_sent=int(f["sel"].size), observations=int(f["obs_kf"].size), call_us=round(call, 1), host_us=round(hst, 1),
                host_over_call=round(hst / call, 2), launches=dict(warm=WARM, timed=REPS))


def from_trace(db_path, runs_path, out_path, csv_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = list(db.execute("select name, duration from kernels order by start"))
    res = json.load(open(runs_path))
    med = lambda v: round(float(np.median(v)) / 1e3, 1)
    for kern, key in (("sim3_correct_kf_kernel", "kf_kernel_us"), ("sim3_correct_pt_kernel", "pt_kernel_us")):
        k = [d for n, d in rows if kern in n]
        o = 0
        for r in res["runs"]:
            o += r["launches"]["warm"]
            r[key] = med(k[o:o + r["launches"]["timed"]]); o += r["launches"]["timed"]
        if o > len(k):
            raise SystemExit(f"trace holds {len(k)} {kern} launches, the runs recorded {o}")
    res["kernel_source"] = "rocprofv3 --kernel-trace of the same script, medians per size (scripts/sim3_correct_profile.py --from-trace)"
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
