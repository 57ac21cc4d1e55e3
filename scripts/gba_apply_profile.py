"""GPU box: time of the map update that follows a global BA (ccm_gba_apply_map) at the three sizes of ccm_slam_amd.gba_apply.SIZES.  Per size a BA handle over
the walk's vertices and the map's landmarks holds the optimised state (created and given one LM iteration outside the timed region); median of interleaved
repetitions (a, b, c, a, b, c, ... on one box):
  handle_us    (a) ccm_gba_apply_map, handle form, host to host: packing, one H2D copy, the launches, one D2H copy, unpacking
  download_us  (b) ccm_ba_download of cameras and landmarks, then ccm_gba_apply_map in the host form
  host_us      (c) ccm_ba_download, then the same arguments through gba_apply_math.h compiled for the host on one thread (ccmh_gba_apply_map_host): what a
               caller can do without this stage, the baseline
All three go through the same ctypes binding, whose cost (array checks, output allocation) is in every figure.  Compare only rows of one run; the margin that
counts as a difference is max - min of host_us over three alternated runs on one box.  Prints one JSON line; --out FILE also writes it there.
Device time, in a run of its own (no counters): `rocprofv3 --kernel-trace --stats -d DIR -o gba -- python scripts/gba_apply_profile.py --out A.json`, then
`python scripts/gba_apply_profile.py --from-trace DIR/gba_results.db --runs A.json --out B.json --stats-csv C.csv`: the trace's three kernels are split by the
launch counts each size recorded; B.json is A.json with their medians added, C.csv the per-kernel summary."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import gba_apply as G, optimizer
from ccm_slam_amd._lib import Context, check, lib

REPS = 15
WARM = 2
K = np.array([458.654, 457.296, 367.215, 248.375])


def ba_problem(f, rng):
    """a BA problem over the walk's cameras and the map's landmarks: every landmark is seen by three cameras near it in camera order (exact projections of the
    scene's state plus a pixel of noise), camera 0 fixed.  Only its size and its device state matter here."""
    cam = np.asarray(f["cam_qt"], np.float64).reshape(-1, 7); pts = np.asarray(f["pt_xyz"], np.float64).reshape(-1, 3)
    n_cam, n_lm = cam.shape[0], pts.shape[0]
    e_pt = np.repeat(np.arange(n_lm), 3).astype(np.int32)
    e_cam = ((np.repeat(rng.integers(0, n_cam, n_lm), 3) + np.tile(np.arange(3), n_lm)) % n_cam).astype(np.int32)
    e_obs = np.tile(K[2:], (e_pt.size, 1)) + rng.normal(0, 30.0, (e_pt.size, 2))
    fixed = np.zeros(n_cam, np.uint8); fixed[0] = 1
    return dict(n_cam=n_cam, n_pt=n_lm, n_edge=int(e_pt.size), cam_qt=cam, cam_fixed=fixed, cam_K=np.tile(K, (n_cam, 1)), pt_xyz=pts, e_cam=e_cam, e_pt=e_pt,
                e_obs=e_obs, e_info=np.ones(e_pt.size), huber_delta=float(np.sqrt(5.991)))


def run(ctx, size):
    n_kf, n_pt = G.SIZES[size]
    f = G.flatten(G.make_scene(seed=200 + n_kf, n_kf=n_kf, n_pt=n_pt))
    prob = ba_problem(f, np.random.default_rng(1))
    ba = optimizer.BAHandle(ctx, prob)
    ba.run(1)
    cam = np.zeros(7 * prob["n_cam"]); pts = np.zeros(3 * prob["n_pt"])
    fh = dict(f, cam_qt=None, pt_xyz=None)

    def download():
        check(lib().ccm_ba_download(ba._h, C.c_void_p(cam.ctypes.data), C.c_void_p(pts.ctypes.data), None), ctx.handle)
        return dict(f, cam_qt=cam, pt_xyz=pts)
    ta, tb, tc = [], [], []
    for i in range(WARM + REPS):
        t = time.perf_counter(); G.apply_map(ctx, fh, ba=ba); a = time.perf_counter() - t
        t = time.perf_counter(); G.apply_map(ctx, download()); b = time.perf_counter() - t
        t = time.perf_counter(); G.apply_map_host(download()); c = time.perf_counter() - t
        if i >= WARM:
            ta.append(a); tb.append(b); tc.append(c)
    ba.close()
    us = lambda v: round(1e6 * float(np.median(v)), 1)
    return dict(size=size, keyframes=int(f["n_kf"]), non_vertex_keyframes=int((f["kf_cam"] < 0).sum()), points=n_pt, cameras=prob["n_cam"], landmarks=prob["n_pt"],
                handle_us=us(ta), download_us=us(tb), host_us=us(tc), host_over_handle=round(us(tc) / us(ta), 2), launches=dict(warm=2 * WARM, timed=2 * REPS))


def from_trace(db_path, runs_path, out_path, csv_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    rows = list(db.execute("select name, duration from kernels order by start"))
    res = json.load(open(runs_path))
    med = lambda v: round(float(np.median(v)) / 1e3, 1)
    for kern, key in (("gba_apply_kf_kernel", "kf_kernel_us"), ("gba_apply_tree_kernel", "tree_kernel_us"), ("gba_apply_pt_kernel", "pt_kernel_us")):
        k = [d for n, d in rows if kern in n]
        o = 0
        for r in res["runs"]:   # two device calls per repetition: the handle form and the host form
            o += r["launches"]["warm"]
            r[key] = med(k[o:o + r["launches"]["timed"]]); o += r["launches"]["timed"]
        if o > len(k):
            raise SystemExit(f"trace holds {len(k)} {kern} launches, the runs recorded {o}")
    res["kernel_source"] = "rocprofv3 --kernel-trace of the same script, medians per size (scripts/gba_apply_profile.py --from-trace)"
    line = json.dumps(res)
    print(line)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    if csv_path:
        by = {}
        for n, d in rows:
            if "gba_apply" in n or "bb_points_out" in n:
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
