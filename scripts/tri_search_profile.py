"""GPU box: host-to-host time of CreateNewMapPoints' SearchForTriangulation for all neighbours of a new keyframe on keyframes of a store, per
workload (tri_search.PROFILE_SIZES: 20 neighbours x 1 000 features, 20 x 2 000, 5 x 1 000, all over about 100 vocabulary nodes, half the features without a map
point).  Routes, interleaved within every repetition (REPS = 200 after WARM = 10), each reported as median and the 10th .. 90th percentile:
    batch_us    cslam::SearchForTriangulationBatch on the device store: the constructor (ONE ccm_tri_search_eval_resident call) and one resolve per neighbour
    call_us     the device entry alone through the Python wrapper (no resolve)
    host_1_us   the same mirror with the host evaluator, one thread (csrc/tri_search_math.h compiled for the host)
    today_us    today's route: cslam::TriangulationBatch (host bucketing, the query descriptors once per neighbour and every neighbour's descriptors uploaded, one
                ccm_hamming_csr_multi launch, the download of every distance) and one resolve per neighbour
Every route resolves under the flags of the build, with the orientation filter.  The routes must return the same matches: asserted.  Also per workload: the matches
found, the queries, the candidates without a map point met, and the bytes the device call moves.  Prints one JSON line; --out FILE also writes it there.

Kernel time: `rocprofv3 --kernel-trace --stats -d DIR -o tri -- python scripts/tri_search_profile.py --device-only`, then
`python scripts/tri_search_profile.py --from-trace DIR/tri_results.db --out profiles/tri_search_profile_traced.json`: the median per workload of tri_search_kernel over
the timed calls of the --device-only mode (WARM + REPS calls per workload, in the order above).  Compare only figures of one invocation on one box."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import fuse_sim3 as fs, kfstore as ks, tri_search as ts
from ccm_slam_amd._lib import Context, _p, host

REPS = 200
WARM = 10
SIZES = list(ts.PROFILE_SIZES)


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


def _install(store, sc, key0=100):
    rec = fs.kf_record(sc["K4"], fs.BOUNDS)
    keys = list(range(key0, key0 + len(sc["kfs"])))
    for key, kf in zip(keys, sc["kfs"]):
        n = kf["desc"].shape[0]
        store.add([key], rec, [0, n], kf["xy"], kf["octave"], kf["desc"])
        store.set_featvec(key, kf["fv"], kf["angle"])
    return keys


def _today(device):
    h = host()
    V, I, F = C.c_void_p, C.c_int, C.c_float
    h.ccmh_tri_batch_create.restype = V
    h.ccmh_tri_batch_create.argtypes = [I, F, I, V, V, V, I, V, V, V, V, V, I, I] + [V] * 11
    h.ccmh_tri_batch_resolve.argtypes = [V, I, V, V, V, F, F, V, V, V]
    h.ccmh_tri_batch_destroy.restype = None
    h.ccmh_tri_batch_destroy.argtypes = [V]

    def run(sc):
        cur, nbs = sc["kfs"][0], sc["kfs"][1:]
        c = np.ascontiguousarray
        keep = []

        def ptrs(arrs):
            arrs = [c(a) for a in arrs]
            keep.extend(arrs)
            return (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        x1, y1 = c(cur["xy"][:, 0]), c(cur["xy"][:, 1])
        nn2 = np.array([k["fv"][0].size for k in nbs], np.int32); N2 = np.array([k["desc"].shape[0] for k in nbs], np.int32)
        hb = h.ccmh_tri_batch_create(device, F(0.6), 1, _p(cur["fv"][0]), _p(cur["fv"][1]), _p(cur["fv"][2]), int(cur["fv"][0].size), _p(cur["has"]), _p(cur["desc"]),
                                     _p(x1), _p(y1), _p(cur["angle"]), int(cur["desc"].shape[0]), len(nbs), ptrs([k["fv"][0] for k in nbs]), ptrs([k["fv"][1] for k in nbs]),
                                     ptrs([k["fv"][2] for k in nbs]), _p(nn2), ptrs([k["has"] for k in nbs]), ptrs([k["desc"] for k in nbs]),
                                     ptrs([k["xy"][:, 0] for k in nbs]), ptrs([k["xy"][:, 1] for k in nbs]), ptrs([k["octave"].astype(np.int32) for k in nbs]),
                                     ptrs([k["angle"] for k in nbs]), _p(N2))
        if not hb:
            raise SystemExit("ccmh_tri_batch_create failed")
        out = []
        for j, k in enumerate(nbs):
            m = np.zeros(cur["desc"].shape[0], np.int32)
            n = h.ccmh_tri_batch_resolve(hb, j, None, None, _p(c(k["F12"].reshape(9))), F(float(k["ex"])), F(float(k["ey"])), _p(sc["level_sigma2"]),
                                         _p(sc["scale_factors"]), _p(m))
            out.append((n, m))
        h.ccmh_tri_batch_destroy(hb)
        return out
    return run


def _jobs(keys, sc):
    cur = sc["kfs"][0]
    return [(keys[0], key, cur["has"], k["has"], k["F12"], k["ex"], k["ey"]) for key, k in zip(keys[1:], sc["kfs"][1:])]


def routes(ctx, store, hstore, name, today):
    sc = ts.profile_scene(**ts.PROFILE_SIZES[name])
    keys = _install(store, sc); _install(hstore, sc)
    cur, nbs = sc["kfs"][0], sc["kfs"][1:]
    has2 = [k["has"] for k in nbs]
    epi = [(k["F12"], k["ex"], k["ey"]) for k in nbs]
    jobs = _jobs(keys, sc)
    sf, s2 = sc["scale_factors"], sc["level_sigma2"]
    info = {}

    def mirror(st, on_host, tag):
        info[tag] = ts.search_for_triangulation_batch(st, keys[0], keys[1:], cur["has"], has2, epi, s2, sf, True, host=on_host)

    def old():
        info["today"] = today(sc)
    r = _interleaved(dict(batch_us=lambda: mirror(store, False, "dev"), call_us=lambda: ts.pair_eval_resident(ctx, store, jobs, sf, s2),
                          host_1_us=lambda: mirror(hstore, True, "host"), today_us=old))
    for st in (store, hstore):
        for k in keys:
            st.erase(k)
    d = info["dev"]
    agree = all(d["nmatches"][j] == info["today"][j][0] == info["host"]["nmatches"][j] and np.array_equal(d["matches12"][j], info["today"][j][1]) and
                np.array_equal(d["matches12"][j], info["host"]["matches12"][j]) for j in range(len(nbs)))
    assert agree, f"{name}: the routes do not return the same matches"
    assert sum(d["nmatches"]) > 10 * len(nbs), f"{name}: too few matches to show anything"
    n1 = int(cur["desc"].shape[0])
    return dict(size=name, neighbours=len(nbs), features=n1, nodes=int(cur["fv"][0].size), nmatches=[int(x) for x in d["nmatches"]], routes_agree=bool(agree),
                queries=int(d["n_query"].sum()), matched_words=int(d["n_match"].sum()), candidates_met=int(d["n_dist"].sum()), down_bytes=4 * n1 * len(nbs) + 12 * len(nbs),
                **r)


def device_only():
    ctx = Context(0)
    store = ks.KeyFrameStore(ctx, 24, 2100)
    for name in SIZES:
        sc = ts.profile_scene(**ts.PROFILE_SIZES[name])
        keys = _install(store, sc)
        jobs = _jobs(keys, sc)
        for _ in range(WARM + REPS):
            ts.pair_eval_resident(ctx, store, jobs, sc["scale_factors"], sc["level_sigma2"])
        for k in keys:
            store.erase(k)
    store.close(); ctx.close()


def from_trace(db_path, out_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    per = WARM + REPS
    d = [x for n, x in db.execute("select name, duration from kernels order by start") if "tri_search_kernel" in n]
    if len(d) != per * len(SIZES):
        raise SystemExit(f"trace holds {len(d)} launches of tri_search_kernel, expected {per * len(SIZES)}")
    rows = []
    for i, name in enumerate(SIZES):
        v = np.array(d[i * per + WARM:(i + 1) * per]) / 1e3
        rows.append(dict(size=name, kernel_us=dict(median=round(float(np.median(v)), 1), p10=round(float(np.percentile(v, 10)), 1), p90=round(float(np.percentile(v, 90)), 1))))
    line = json.dumps(dict(kernel_source=f"rocprofv3 --kernel-trace --stats of scripts/tri_search_profile.py --device-only, {REPS} timed launches each", rows=rows))
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
    store = ks.KeyFrameStore(ctx, 24, 2100); hstore = ks.KeyFrameStore(None, 24, 2100)
    today = _today(0)
    rows = [routes(ctx, store, hstore, name, today) for name in SIZES]
    store.close(); hstore.close(); ctx.close()
    line = json.dumps(dict(reps=REPS, warm=WARM, rows=rows))
    print(line)
    if arg("--out"):
        with open(arg("--out"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
