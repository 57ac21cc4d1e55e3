"""GPU box: host-to-host time of the triangulation of new map points (ccm_triangulate_pairs, cslam::NewMapPointBatch) for 20 neighbours of
50 / 100 / 400 matches each, median of repeated runs:
  one_launch    one ccm_triangulate_pairs over all 20 groups (what NewMapPointBatch does when it is built)
  per_neighbour 20 ccm_triangulate_pairs calls of one group each, back to back
  host          the same matches through tri_pair compiled for the host, on one thread (ccmh_triangulate_pairs_host)
and the hit rate of the prediction of NewMapPointBatch on a multi-neighbour keyframe scene whose stand-in matcher lets a later feature take over a
claimed candidate (ccm_slam_amd.triangulate.make_keyframe_scene).  Compare only rows of one run: all three are measured on the same box.
Prints one JSON line; --out FILE also writes it there.  Each run records how many triangulate_kernel launches it made, in order.
Device time: run the script under `rocprofv3 --kernel-trace --stats -d DIR -o tri -- python scripts/triangulate_profile.py --out A.json`, then
`python scripts/triangulate_profile.py --from-trace DIR/tri_results.db --runs A.json --out B.json --stats-csv C.csv`: the trace's triangulate_kernel
dispatches are split by those counts, B.json is A.json with the median kernel time of each phase added, C.csv the per-kernel summary."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import triangulate as T
from ccm_slam_amd._lib import Context

REPS = 30
WARM = 3


def _timed(f):
    for _ in range(WARM):
        f()
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return round(1e6 * float(np.median(ts)), 1)


def run(ctx, n):
    sc = T.make_pair_scene(seed=1000 + n, S=20, n_pairs=n)
    args = T.flat(sc)
    off = sc["pair_off"]
    groups = [(sc["cam1"], sc["cam2"][s:s + 1], np.array([0, off[s + 1] - off[s]], np.int32), sc["xy"][off[s]:off[s + 1]], sc["oct"][off[s]:off[s + 1]]) + args[5:]
              for s in range(20)]
    one = _timed(lambda: T.triangulate_pairs(ctx, *args))
    per = _timed(lambda: [T.triangulate_pairs(ctx, *g) for g in groups])
    host = _timed(lambda: T.triangulate_pairs_host(*args))
    st, _, _ = T.triangulate_pairs(ctx, *args)
    return dict(neighbours=20, matches_per_neighbour=n, matches=int(off[-1]), accepted=int((st == 0).sum()), one_launch_us=one, per_neighbour_us=per, host_us=host,
                launches=dict(one_warm=WARM, one_timed=REPS, per_warm=20 * WARM, per_timed=20 * REPS, tail=1))


def hit_rate():
    out = []
    for seed, disjoint in ((0, False), (1, False), (5, True)):
        sc = T.make_keyframe_scene(seed=seed, S=20, n_feat=600, disjoint=disjoint)
        has1 = np.zeros(600, np.uint8)
        b = T.NewMapPoints(0, sc["cam1"], sc["keys1"], sc["cam2"], sc["keys2"], [T.resolve_candidates(c, has1) for c in sc["cands"]], sc["sigma2"], sc["sf"],
                           sc["sigma2"], sc["sf"], sc["ratio"])
        for j in range(20):
            pairs = T.resolve_candidates(sc["cands"][j], has1)
            st, _, _ = b.points(j, pairs)
            has1[pairs[st == 0, 0]] = 1
        predicted, hits, misses = b.stats()
        b.close()
        out.append(dict(seed=seed, disjoint=disjoint, predicted=predicted, hits=hits, misses=misses, hit_rate=round(hits / max(hits + misses, 1), 4)))
    return out


def from_trace(db_path, runs_path, out_path, csv_path):
    """split the trace's triangulate_kernel dispatches (in start order) by the launch counts each run recorded; add the median of each phase"""
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = list(db.execute("select name, duration from kernels order by start"))
    res = json.load(open(runs_path))
    k = [d for n, d in rows if "triangulate_kernel" in n]
    o = 0
    med = lambda v: round(float(np.median(v)) / 1e3, 1)
    for r in res["runs"]:
        L = r["launches"]
        o += L["one_warm"]
        r["one_launch_kernel_us"] = med(k[o:o + L["one_timed"]]); o += L["one_timed"]
        o += L["per_warm"]
        r["per_neighbour_kernel_us"] = med(k[o:o + L["per_timed"]]); o += L["per_timed"] + L["tail"]
    if o > len(k):
        raise SystemExit(f"trace holds {len(k)} triangulate_kernel launches, the runs recorded at least {o}")
    res["kernel_source"] = "rocprofv3 --kernel-trace of the same script, medians per phase (scripts/triangulate_profile.py --from-trace)"
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
    runs = [run(ctx, n) for n in (50, 100, 400)]
    ctx.close()
    line = json.dumps(dict(reps=REPS, runs=runs, prediction=hit_rate()))
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
