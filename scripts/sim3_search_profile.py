"""GPU box: host-to-host time of ComputeSim3's two projected searches on keyframes of a store, per workload:
  loop    SearchByProjection: one keyframe of about 1 000 features x 8 000 loop points;  SearchBySim3: two keyframes with about 800 live points each
  small   SearchByProjection: 2 000 points;                                              SearchBySim3: 300 live points each
Per search and workload, three routes, interleaved within every repetition (REPS = 200 after WARM = 10), each reported as median and the 10th .. 90th percentile:
    device_us   the mirror on the device store: cslam::Sim3ProjectionSearch (ONE ccm_sim3_project_eval_resident call, then resolve) / cslam::SearchBySim3Batch (ONE
                ccm_sim3_pair_eval_resident call, then the agreement step)
    call_us     the device entry alone through the Python wrapper (no resolve, no packing of the live points)
    host_1_us   the same mirror with the host evaluator, one thread (csrc/fuse_math.h compiled for the host)
    today_us    today's route: the projection and its gates on the host (timed as the host evaluator on a keyframe WITHOUT features: gates, PredictScale and the cell
                range, nothing else), then cslam::ORBmatcher::ProjectedSearch on the device context, whose Hamming distances are one ccm_hamming_csr launch
                (claims and the skip of matched features for SearchByProjection; two calls and the agreement step for SearchBySim3)
Also per workload: the points resolve evaluated again (n_reeval) and the matches found.  Prints one JSON line; --out FILE also writes it there.

Kernel time: `rocprofv3 --kernel-trace --stats -d DIR -o ss -- python scripts/sim3_search_profile.py --device-only`, then
`python scripts/sim3_search_profile.py --from-trace DIR/ss_results.db --out profiles/sim3_search_profile_traced.json`: the median per workload of
proj_sim3_resident_kernel and sim3_pair_resident_kernel over the timed calls of the --device-only mode (WARM + REPS calls per kernel and workload, in the order
above).  Compare only figures of one invocation on one box."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import fuse_sim3 as fs, kfstore as ks, sim3_search as ss
from ccm_slam_amd._lib import Context, _p, host

REPS = 200
WARM = 10
SIZES = list(ss.PROFILE_SIZES)
c = np.ascontiguousarray


def _interleaved(fns):
    for _ in range(WARM):
        for f in fns.values():
            f()
    ts = {k: [] for k in fns}
    for _ in range(REPS):
        for k, f in fns.items():
            t = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t)
    us = lambda v, q: round(1e6 * float(np.percentile(v, q)), 1)
    return {k: dict(median=us(v, 50), p10=us(v, 10), p90=us(v, 90)) for k, v in ts.items()}


def _today(device):
    h = host()
    V, I, F = C.c_void_p, C.c_int, C.c_float
    h.ccmh_projected_window_search.argtypes = [I, V, V, V, V, I, F, F, F, F, V, V, I, V, V, V, V, V, F, I, I, V, I, V, V, V]

    def search(kf, sf, isig, valid, u, v, level, pdesc, th, dist_th, matched, claim):
        n = int(valid.size)
        bi = np.zeros(n, np.int32); bd = np.zeros(n, np.int32)
        return h.ccmh_projected_window_search(device, _p(kf[0]), _p(kf[1]), _p(kf[2]), _p(kf[3]), int(kf[0].size), *[C.c_float(b) for b in fs.BOUNDS], _p(sf), _p(isig), n,
                                              _p(valid), _p(u), _p(v), _p(level), _p(pdesc), C.c_float(th), 0, dist_th, _p(matched), int(claim), None, _p(bi), _p(bd)), bi
    return search


def _kf_arrays(sc, k):
    a, b = int(sc.feat_off[k]), int(sc.feat_off[k + 1])
    xy = sc.feat_xy.reshape(-1, 2)[a:b]
    return c(xy[:, 0]), c(xy[:, 1]), c(sc.feat_octave[a:b].astype(np.int32)), c(sc.feat_desc.reshape(-1, 32)[a:b])


def _empty_like(sc, k):
    """keyframe k's record without features, under a key of its own: what is left of a pair there is the projection, its gates and the cell range"""
    z = np.zeros(0, np.float32)
    return sc.rec.reshape(-1, 10)[k:k + 1], np.array([0, 0], np.int32), z, np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(fs.CELLS + 1, np.int32), np.zeros(0, np.int32)


def projection_routes(ctx, store, hstore, name, today):
    sc, m0 = ss.projection_profile_scene(ss.PROFILE_SIZES[name]["points"])
    key, ekey = 10, 11
    for st in (store, hstore):
        st.add_scene([key], sc, grid=True)
        st.add([ekey], *_empty_like(sc, 0))
    matched0 = np.where(m0 > 0, 1_000_000, -1).astype(np.int32)
    isig = np.ones(sc.nlevels, np.float32)
    kf = _kf_arrays(sc, 0)
    info = {}

    def mirror(st, on_host):
        s = ss.Sim3ProjectionSearch(st, key, sc, m0, host=on_host)
        n = s.resolve(matched0)[0]
        info.update(nmatches=n, n_reeval=s.n_reeval())
        s.close()

    def old():
        g = ss.project_eval_resident_host(hstore, [ekey], sc, [np.zeros(0, np.uint8)], want_uv=True)
        t = fs.unpack_table(g["table"][0])
        n, _ = today(kf, sc.scale_factors, isig, c((t["status"] >= 4).astype(np.uint8)), c(g["uv"][0, :, 0]), c(g["uv"][0, :, 1]), c(t["level"]), sc.pt_desc, sc.th, 50,
                     matched0.copy(), True)
        info["today_nmatches"] = n
    r = _interleaved(dict(device_us=lambda: mirror(store, False), call_us=lambda: ss.project_eval_resident(ctx, store, [key], sc, [m0]),
                          host_1_us=lambda: mirror(hstore, True), today_us=old))
    for st in (store, hstore):
        st.erase(key); st.erase(ekey)
    info["routes_agree"] = info["nmatches"] == info["today_nmatches"]
    return dict(search="SearchByProjection", size=name, features=int(sc.feat_off[1]), points=sc.P, **info, **r)


def pair_routes(ctx, store, hstore, name, today):
    p = ss.pair_profile_scene(ss.PROFILE_SIZES[name]["live"])
    kfs = p["kfs"]
    keys, ekeys = [20, 21], [22, 23]
    for st in (store, hstore):
        st.add_scene(keys, kfs, grid=True)
        for k in (0, 1):
            st.add([ekeys[k]], *_empty_like(kfs, k))
    s1, s2 = p["side1"], p["side2"]
    sf = kfs.scale_factors; isig = np.ones(kfs.nlevels, np.float32)
    kf = [_kf_arrays(kfs, 0), _kf_arrays(kfs, 1)]
    # the packed points of both directions, as the mirror packs them
    a1 = p["matches12_in"] >= 0
    a2 = np.zeros(s2.N, bool); a2[p["matches12_in"][a1]] = True
    i1 = np.flatnonzero((s1.live > 0) & ~a1); i2 = np.flatnonzero((s2.live > 0) & ~a2)
    sR12, sR21, t21 = ss.derive(p["s12"], p["R12"], p["t12"])
    K4 = kfs.rec[:4]
    take = lambda s, i: (s.pos.reshape(-1, 3)[i], s.min_dist[i], s.max_dist[i], s.desc.reshape(-1, 32)[i])
    cat = lambda j: np.concatenate([take(s1, i1)[j], take(s2, i2)[j]])
    jobs = lambda kf_of: [(kf_of[1], K4, s1.pose, np.concatenate([sR21, t21]), 0, i1.size), (kf_of[0], K4, s2.pose, np.concatenate([sR12, p["t12"]]), i1.size, i2.size)]
    ps = ss.PairScene(kfs, p["th"], cat(0), cat(1), cat(2), cat(3), jobs([0, 1]))
    info = {}

    def mirror(st, on_host):
        info["nFound"] = ss.search_by_sim3(st, keys[0], keys[1], s1, s2, p["s12"], p["R12"], p["t12"], p["matches12_in"], sf, p["th"], host=on_host, log_sf=kfs.log_sf)["nFound"]

    def old():
        g = ss.pair_eval_resident_host(hstore, ekeys, ps, want_uv=True)
        t = fs.unpack_table(g["table"]); valid = (t["status"] >= 4).astype(np.uint8)
        vn = []
        for j, (tgt, idx) in enumerate(((1, i1), (0, i2))):
            s = slice(int(g["off"][j]), int(g["off"][j + 1]))
            _, bi = today(kf[tgt], sf, isig, c(valid[s]), c(g["uv"][s, 0]), c(g["uv"][s, 1]), c(t["level"][s]), c(ps.pt_desc.reshape(-1, 32)[s]), p["th"], 100, None, False)
            full = -np.ones((s1.N, s2.N)[j], np.int32); full[idx] = bi
            vn.append(full)
        k = np.flatnonzero(vn[0] >= 0)
        info["today_nFound"] = int((vn[1][vn[0][k]] == k).sum())
    r = _interleaved(dict(device_us=lambda: mirror(store, False), call_us=lambda: ss.pair_eval_resident(ctx, store, keys, ps), host_1_us=lambda: mirror(hstore, True),
                          today_us=old))
    for st in (store, hstore):
        for k in keys + ekeys:
            st.erase(k)
    info["routes_agree"] = info["nFound"] == info["today_nFound"]
    return dict(search="SearchBySim3", size=name, features=[s1.N, s2.N], points=[int(i1.size), int(i2.size)], **info, **r)


def device_only():
    ctx = Context(0)
    store = ks.KeyFrameStore(ctx, 4, 1100)
    for name in SIZES:
        sc, m0 = ss.projection_profile_scene(ss.PROFILE_SIZES[name]["points"])
        store.add_scene([10], sc, grid=True)
        for _ in range(WARM + REPS):
            ss.project_eval_resident(ctx, store, [10], sc, [m0])
        store.erase(10)
    for name in SIZES:
        p = ss.pair_profile_scene(ss.PROFILE_SIZES[name]["live"])
        store.add_scene([20, 21], p["kfs"], grid=True)
        for _ in range(WARM + REPS):
            ss.search_by_sim3(store, 20, 21, p["side1"], p["side2"], p["s12"], p["R12"], p["t12"], p["matches12_in"], p["kfs"].scale_factors, p["th"], log_sf=p["kfs"].log_sf)
        store.erase(20); store.erase(21)
    store.close(); ctx.close()


def from_trace(db_path, out_path):
    import sqlite3
    db = sqlite3.connect(db_path)
    per = WARM + REPS
    rows = []
    for kernel, search in (("proj_sim3_resident_kernel", "SearchByProjection"), ("sim3_pair_resident_kernel", "SearchBySim3")):
        d = [x for n, x in db.execute("select name, duration from kernels order by start") if kernel in n]
        if len(d) != per * len(SIZES):
            raise SystemExit(f"trace holds {len(d)} launches of {kernel}, expected {per * len(SIZES)}")
        for i, name in enumerate(SIZES):
            v = np.array(d[i * per + WARM:(i + 1) * per]) / 1e3
            rows.append(dict(search=search, size=name, kernel_us=dict(median=round(float(np.median(v)), 1), p10=round(float(np.percentile(v, 10)), 1),
                                                                      p90=round(float(np.percentile(v, 90)), 1))))
    line = json.dumps(dict(kernel_source=f"rocprofv3 --kernel-trace --stats of scripts/sim3_search_profile.py --device-only, {REPS} timed launches each", rows=rows))
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
    store = ks.KeyFrameStore(ctx, 8, 1100); hstore = ks.KeyFrameStore(None, 8, 1100)
    today = _today(0)
    rows = []
    for name in SIZES:
        rows.append(projection_routes(ctx, store, hstore, name, today))
        rows.append(pair_routes(ctx, store, hstore, name, today))
    store.close(); hstore.close(); ctx.close()
    line = json.dumps(dict(reps=REPS, warm=WARM, rows=rows))
    print(line)
    if arg("--out"):
        with open(arg("--out"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
