"""GPU box: host-to-host time of the refresh of map points after a map stage (ComputeDistinctiveDescriptors + UpdateNormalAndDepth) on a store of 21
keyframes, per workload (mappoint.PROFILE_SIZES: 1 000 points x 2 observations as CreateNewMapPoints leaves them, 1 000 x mean 6 as the tail of SearchInNeighbors,
5 000 x mean 15 with one point in a hundred between 100 and 200 observations as a server after a Fuse).  Routes, interleaved within every repetition (REPS = 200
after WARM = 10), each reported as median and the 10th .. 90th percentile, all through the Python wrappers with the profiler off:
    refresh_us  ccm_mappoint_refresh_resident: one upload of 8 bytes per observation, ONE launch, one download
    today_us    today's route: the host gather of one 32-byte descriptor row per observation and of the reference levels, ccm_distinctive_descriptors and
                ccm_update_normal_and_depth (two calls, two uploads)
    host_1_us   the host evaluator on one thread (csrc/mappoint_math.h compiled for the host) on the shadows of a host-only store
The routes must return the same results: asserted.  Also per workload: the observations, the largest list, the points per size class and the bytes each device route
uploads.  Prints one JSON line; --out FILE also writes it there.

Kernel time: `rocprofv3 --kernel-trace --stats -d DIR -o mpr -- python scripts/mappoint_refresh_profile.py --device-only`, then
`python scripts/mappoint_refresh_profile.py --from-trace DIR/mpr_results.db --out profiles/mappoint_refresh_profile_traced.json`: the median per workload of
mappoint_refresh_kernel, and of distinctive_kernel and frame_normal_depth_kernel, over the timed calls of the --device-only mode (WARM + REPS calls per workload and
route, in the order above).  Compare only figures of one invocation on one box."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import frame, kfstore as ks, mappoint as mp, matcher
from ccm_slam_amd._lib import Context

REPS = 200
WARM = 10
SIZES = list(mp.PROFILE_SIZES)
KERNELS = ("mappoint_refresh_kernel", "distinctive_kernel", "frame_normal_depth_kernel")


def _interleaved(fns):
    for _ in range(WARM):
        for f in fns.values():
            f()
    t_ = {k: [] for k in fns}
    for _ in range(REPS):
        for k, f in fns.items():
            t = time.perf_counter()
            f()
            t_[k].append(time.perf_counter() - t)
    us = lambda v, q: round(1e6 * float(np.percentile(v, q)), 1)
    return {k: dict(median=us(v, 50), p10=us(v, 10), p90=us(v, 90)) for k, v in t_.items()}


def _today(ctx, sc):
    """today's route on the caller's own arrays: what the caller holds is one descriptor matrix and one octave array per keyframe"""
    # the keyframes' arrays one after the other stand for the caller's memory (not timed); the gather is one indexed copy per call
    descs = np.concatenate([kf["desc"] for kf in sc["kfs"]]); octs = np.concatenate([kf["octave"] for kf in sc["kfs"]])
    base = np.concatenate([[0], np.cumsum([kf["octave"].size for kf in sc["kfs"]])]).astype(np.int64)
    okf, ofeat, off = sc["obs_kf"], sc["obs_feat"], sc["obs_off"]

    def run():
        rows = descs[base[okf] + ofeat]                              # the gather of one 32-byte row per observation
        level = octs[base[sc["ref_kf"]] + sc["ref_feat"]].astype(np.int32)
        best = matcher.distinctive_descriptors(ctx, rows, off)
        nrm, dmin, dmax = frame.update_normal_and_depth(ctx, sc["pos"], off, okf, sc["kf_center"], sc["ref_kf"], level, sc["scale_factors"], sc["normal"], sc["min_dist"],
                                                        sc["max_dist"])
        return dict(best_obs=best, best_desc=rows[off[:-1] + best], normal=nrm, min_dist=dmin, max_dist=dmax)
    return run


def _same(a, b):
    bits = lambda x: np.ascontiguousarray(x, np.float32).reshape(-1).view(np.uint32)
    return bool(np.array_equal(a["best_obs"], b["best_obs"]) and np.array_equal(a["best_desc"], b["best_desc"]) and
                all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("normal", "min_dist", "max_dist")))


def _scene(name):
    sc = mp.profile_scene(**mp.PROFILE_SIZES[name])
    n = np.diff(sc["obs_off"])
    assert n.min() >= 1 and n.max() <= mp.MAX_OBS
    return sc, n


def routes(ctx, name):
    sc, n = _scene(name)
    store = ks.KeyFrameStore(ctx, sc["K"], sc["max_feat"]); hstore = ks.KeyFrameStore(None, sc["K"], sc["max_feat"])
    mp.add_scene(store, sc); mp.add_scene(hstore, sc)
    args = mp.call_args(sc)
    seeds = dict(normal=sc["normal"], min_dist=sc["min_dist"], max_dist=sc["max_dist"])
    today = _today(ctx, sc)
    info = {}

    def new():
        info["dev"] = mp.refresh_resident(ctx, store, *args, **seeds)

    def old():
        info["today"] = today()

    def on_host():
        info["host"] = mp.refresh_host(hstore, *args, **seeds)
    r = _interleaved(dict(refresh_us=new, today_us=old, host_1_us=on_host))
    store.close(); hstore.close()
    agree = _same(info["dev"], info["today"]) and _same(info["dev"], info["host"]) and np.array_equal(info["dev"]["status"], info["host"]["status"])
    assert agree, f"{name}: the routes do not return the same results"
    assert (info["dev"]["status"] == (mp.DESC | mp.NORMAL_DEPTH)).all(), name
    M, P = int(sc["obs_off"][-1]), int(n.size)
    return dict(size=name, points=P, observations=M, max_obs=int(n.max()), classes={"<=8": int((n <= 8).sum()), "<=16": int(((n > 8) & (n <= 16)).sum()),
                                                                                       "<=32": int(((n > 16) & (n <= 32)).sum()), ">32": int((n > 32).sum())},
                routes_agree=bool(agree), up_bytes_refresh=8 * M + 4 * (P + 1) + 4 * 3 * P + 4 * 3 * P + 4 * 5 * P + 12 * sc["K"] + 4 * sc["scale_factors"].size,
                up_bytes_today=32 * M + 4 * (P + 1) + 4 * M + 4 * (P + 1) + 4 * 3 * P + 4 * 2 * P + 4 * 5 * P + 12 * sc["K"] + 4 * sc["scale_factors"].size, **r)


def device_only():
    ctx = Context(0)
    for name in SIZES:
        sc, _ = _scene(name)
        store = ks.KeyFrameStore(ctx, sc["K"], sc["max_feat"])
        mp.add_scene(store, sc)
        args = mp.call_args(sc)
        today = _today(ctx, sc)
        for _ in range(WARM + REPS):
            mp.refresh_resident(ctx, store, *args)
        for _ in range(WARM + REPS):
            today()
        store.close()
    ctx.close()


def from_trace(db_path, out_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    per = WARM + REPS
    launches = list(db.execute("select name, duration from kernels order by start"))
    rows = [dict(size=name) for name in SIZES]
    for kern in KERNELS:
        d = [x for n, x in launches if kern in n]
        if len(d) != per * len(SIZES):
            raise SystemExit(f"trace holds {len(d)} launches of {kern}, expected {per * len(SIZES)}")
        for i in range(len(SIZES)):
            v = np.array(d[i * per + WARM:(i + 1) * per]) / 1e3
            rows[i][kern + "_us"] = dict(median=round(float(np.median(v)), 1), p10=round(float(np.percentile(v, 10)), 1), p90=round(float(np.percentile(v, 90)), 1))
    line = json.dumps(dict(kernel_source=f"rocprofv3 --kernel-trace --stats of scripts/mappoint_refresh_profile.py --device-only, {REPS} timed launches each", rows=rows))
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


def main():
    arg = lambda k: sys.argv[sys.argv.index(k) + 1] if k in sys.argv else None
    if "--device-only" in sys.argv:
        return device_only()
    if "--from-trace" in sys.argv:
        return from_trace(arg("--from-trace"), arg("--out"))
    ctx = Context(0)
    rows = [routes(ctx, name) for name in SIZES]
    ctx.close()
    line = json.dumps(dict(reps=REPS, warm=WARM, rows=rows))
    print(line)
    if arg("--out"):
        with open(arg("--out"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
