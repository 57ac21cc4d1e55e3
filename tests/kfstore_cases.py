"""Cases shared by tests/test_kfstore_cpu.py, tests/test_kfstore_gpu.py and tests/test_fuse_resident_gpu.py (no test lives here).

grid_cases(): keyframes (xy, rec) whose grid is built by the store and compared with kfstore.build_grid_keyframe, the literal replay of KeyFrame::AssignFeaturesToGrid.
planted_roundings(): keypoints on and beside the rounding boundaries of KeyFrame::PosInGrid with both inverses 0.125, so that (x - 0) * 0.125 is exact in f32 and the
expected cell follows from exact arithmetic.
bookkeeping_keyframes(): four small keyframes A, B, C, D (D with fewer features than B) for the slot-reuse sequence.
lockstep_*: a walk of resolve calls through two mirrors at once, between which the map changes; both must answer alike.
"""
from fractions import Fraction

import numpy as np

from ccm_slam_amd import fuse_sim3 as fs, kfstore as ks, synth

f32 = np.float32
K4 = np.array(synth.EUROC_K, f32)
REC = fs.kf_record(K4, fs.BOUNDS)


def rec_with(min_x=0, min_y=0, w_inv=None, h_inv=None):
    r = REC.copy()
    r[4] = min_x; r[5] = min_y
    if w_inv is not None:
        r[8] = w_inv
    if h_inv is not None:
        r[9] = h_inv
    return r


EIGHTH = rec_with(w_inv=0.125, h_inv=0.125)


def _beside(v):
    v = f32(v)
    return [np.nextafter(v, f32(-1e9)), v, np.nextafter(v, f32(1e9))]


def planted_roundings():
    """(xy (n, 2), expected cell per keypoint or -1): t = x / 8 and y / 8 exactly"""
    pts = []
    for t in (-0.5, 0.5, 73.5, 74.5):
        pts += [(x, 8.0) for x in _beside(8 * t)]
    for t in (-0.5, 0.5, 46.5, 47.5):
        pts += [(8.0, y) for y in _beside(8 * t)]
    xy = np.array(pts, f32)

    def pos(c, n):      # round half away from zero of c / 8 in exact arithmetic
        t = Fraction(float(c)) / 8
        p = int(abs(t) + Fraction(1, 2)) * (1 if t >= 0 else -1)
        return p if 0 <= p < n else None
    cells = []
    for x, y in xy:
        px, py = pos(x, 75), pos(y, 48)
        cells.append(-1 if px is None or py is None else px * 48 + py)
    return xy, np.array(cells)


def grid_cases():
    """[(name, xy (n, 2) f32, rec[10])]"""
    rng = np.random.default_rng(21)
    out = []
    sc = fs.make_scene(2, 4, n_feat=1000, seed=0)
    for k in range(2):
        a, b = int(sc.feat_off[k]), int(sc.feat_off[k + 1])
        out.append((f"make_scene keyframe {k}", sc.feat_xy[2 * a:2 * b].reshape(-1, 2), sc.rec[10 * k:10 * k + 10]))
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        out.append((f"n = {n}", np.stack([rng.uniform(0, 752, n), rng.uniform(0, 480, n)], 1).astype(f32), REC))
    out.append(("300 features in one cell", (np.array([300.0, 200.0]) + rng.uniform(-2, 2, (300, 2))).astype(f32), REC))
    two = np.zeros((301, 2), f32); two[0::2] = (100.0, 100.0); two[1::2] = (600.0, 400.0)
    out.append(("two cells alternating", two, REC))
    lo = rec_with(-17, -9, f32(75) / f32(752 + 17), f32(48) / f32(480 + 9))
    out.append(("bounds -17, -9", np.stack([rng.uniform(-25, 760, 500), rng.uniform(-15, 490, 500)], 1).astype(f32), lo))
    out.append(("planted roundings", planted_roundings()[0], EIGHTH))
    bad = np.array([[np.nan, 10], [10, np.nan], [np.inf, 10], [10, -np.inf], [-np.inf, np.inf], [3e38, 10], [10, -3e38], [100, 100], [1e10, 1e10]], f32)
    out.append(("NaN, Inf and huge coordinates", bad, REC))
    return out


def feats(xy, seed=0):
    """octaves and descriptors for n keypoints"""
    rng = np.random.default_rng(seed)
    n = len(xy)
    return rng.integers(0, 8, n).astype(np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)


def add_one(store, key, xy, rec, grid=None, seed=0):
    oc, de = feats(xy, seed)
    store.add([key], rec, [0, len(xy)], xy, oc, de, *(grid if grid is not None else (None, None)))


def same_grid(got, xy, rec, tag):
    off, idx = ks.build_grid_keyframe(xy, rec)
    assert got["n"] == len(xy) and got["n_in"] == off[-1] == idx.size, tag
    assert np.array_equal(got["cell_off"], off), tag
    assert np.array_equal(got["cell_idx"], idx), tag


def bookkeeping_keyframes():
    rng = np.random.default_rng(4)
    out = {}
    for name, n in (("A", 70), ("B", 130), ("C", 5), ("D", 40)):
        out[name] = np.stack([rng.uniform(0, 752, n), rng.uniform(0, 480, n)], 1).astype(f32)
    return out


def bookkeeping_sequence(store):
    """add A, B, C; erase B; add D (fewer features) into B's slot; get of each key"""
    kf = bookkeeping_keyframes()
    oc = {k: feats(v, i) for i, (k, v) in enumerate(kf.items())}
    cat = lambda names, j: np.concatenate([(kf[n] if j == 0 else oc[n][j - 1]).reshape(-1) for n in names])
    names = ["A", "B", "C"]
    off = np.concatenate([[0], np.cumsum([len(kf[n]) for n in names])])
    store.add([1, 2, 3], np.tile(REC, 3), off, cat(names, 0), cat(names, 1), cat(names, 2))
    assert store.count() == (3, 1)
    for key, n in ((1, "A"), (2, "B"), (3, "C")):
        same_grid(store.get(key), kf[n], REC, n)
    store.erase(2)
    store.erase(77)      # an unknown key: a no-op
    assert store.count() == (2, 2)
    add_one(store, 4, kf["D"], REC, seed=3)
    assert store.count() == (3, 1)
    for key, n in ((1, "A"), (4, "D"), (3, "C")):
        same_grid(store.get(key), kf[n], REC, n + " after the reuse")
    return kf


def refusals(store):
    """every refusal of ccm_kfstore_add on a store of 4 slots x 256 features that holds keys 1, 3, 4; the store is unchanged after each"""
    rng = np.random.default_rng(6)
    before = {k: store.get(k) for k in (1, 3, 4)}
    xy = np.stack([rng.uniform(0, 752, 300), rng.uniform(0, 480, 300)], 1).astype(f32)
    oc, de = feats(xy)
    E = ks.StoreError

    def refused(code, keys, n_each, **kw):
        n = list(n_each)
        off = np.concatenate([[0], np.cumsum(n)])
        F = int(off[-1])
        a = dict(rec=np.tile(REC, len(n)), feat_off=off, feat_xy=xy[:F], feat_octave=oc[:F], feat_desc=de[:F])
        a.update(kw)
        try:
            store.add(keys, a["rec"], a["feat_off"], a["feat_xy"], a["feat_octave"], a["feat_desc"], a.get("cell_off"), a.get("cell_idx"))
        except E as e:
            assert e.code == code, (keys, e.code, code)
        else:
            raise AssertionError(f"not refused: {keys}")
        assert store.count() == (3, 1)
        for k, g in before.items():
            now = store.get(k)
            assert now["n"] == g["n"] and np.array_equal(now["cell_off"], g["cell_off"]) and np.array_equal(now["cell_idx"], g["cell_idx"])

    refused(ks.E_STATE, [3], [10])                      # a live key
    refused(ks.E_STATE, [9, 9], [10, 10])               # a key repeated within the call
    refused(ks.E_STATE, [8, 9], [10, 10])               # fewer free slots than keyframes: nothing added
    refused(ks.E_ARG, [9], [257])                       # more than max_feat features
    g = ks.build_grid_keyframe(xy[:10], REC)
    refused(ks.E_ARG, [9], [10], cell_off=g[0])         # one grid pointer without the other
    off = g[0].copy(); off[-1] = 11
    refused(ks.E_ARG, [9], [10], cell_off=off, cell_idx=np.concatenate([g[1], [0]]))      # a grid that ends beyond the feature count
    idx = g[1].copy(); idx[3] = 10
    refused(ks.E_ARG, [9], [10], cell_off=g[0], cell_idx=idx)                              # a cell_idx outside the keyframe
    off = g[0].copy(); j = int(np.flatnonzero(np.diff(off) > 0)[0]); off[j + 1] = off[j] - 1
    refused(ks.E_ARG, [9], [10], cell_off=off, cell_idx=g[1])                              # a cell_off that decreases
    refused(ks.E_ARG, [9], [10], feat_off=np.array([1, 11]))                               # feat_off does not start at 0
    try:
        store.get(2)
    except E as e:
        assert e.code == ks.E_ARG
    else:
        raise AssertionError("get of an erased key")
    # a grid that ends BELOW the feature count is legal
    short = (np.minimum(g[0], 7).astype(np.int32), g[1][:7])
    add_one(store, 9, xy[:10], REC, grid=short)
    got = store.get(9)
    assert (got["n"], got["n_in"]) == (10, 7) and np.array_equal(got["cell_idx"], short[1]) and np.array_equal(got["cell_off"], short[0])
    store.erase(9)


def same_result(got, want, tag, keys=("table", "n_valid", "n_hit")):
    for k in keys:
        assert np.array_equal(got[k], want[k]), (tag, k)
    if "uv" in want and "uv" in got:
        assert np.array_equal(np.asarray(got["uv"]).view(np.uint32), np.asarray(want["uv"]).view(np.uint32)), (tag, "uv")


def lockstep_sim3(a, b, K, P, pdesc, kdesc_of, between=None):
    """K resolve calls through the mirrors a and b, between which the map changes as in tests/test_fuse_sim3_cpu.py's walk; between(k) runs after call k.
    Returns the total number of re-evaluated pairs."""
    rng = np.random.default_rng(77)
    now = np.ascontiguousarray(pdesc).reshape(P, 32).copy()
    skip = np.zeros(P, np.uint8)
    for k in range(K):
        ra, rb = a.resolve(k, skip, now), b.resolve(k, skip, now)
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2]), k
        assert a.n_reeval() == b.n_reeval(), k
        fused = np.flatnonzero(ra[1] >= 0)
        now[fused[0::3]] = kdesc_of(k)[ra[1][fused[0::3]]]
        skip[fused[1::3]] = 1
        skip[rng.choice(P, min(15, P), replace=False)] = 1
        if between:
            between(k)
    return a.n_reeval()


def lockstep_pose(a, b, calls, P1, n_pred, n_pool, sc, kdesc, between=None):
    """the SearchInNeighbors walk of tests/test_fuse_pose_cpu.py through two mirrors at once: the calls of the first loop, then the call on the current keyframe
    with shuffled candidates, unpredicted ones and changed descriptors among them"""
    rng = np.random.default_rng(77)
    now = sc.pt_desc.reshape(-1, 32)[:P1].copy()
    skip = np.zeros(P1, np.uint8)
    for c in range(len(calls)):
        ra, rb = a.resolve(c, skip, now), b.resolve(c, skip, now)
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2]), c
        assert a.n_reeval() == b.n_reeval(), c
        fused = np.flatnonzero(ra[1] >= 0)
        now[fused[0::3]] = kdesc[ra[1][fused[0::3]]]
        skip[fused[1::3]] = 1
        skip[rng.choice(P1, 15, replace=False)] = 1
        if between:
            between(c)
    pool = sc.pt_desc.reshape(-1, 32)[P1:]
    cand = np.concatenate([rng.choice(n_pred, min(1500, n_pred), replace=False), n_pred + rng.choice(n_pool - n_pred, 60, replace=False)])
    rng.shuffle(cand)
    slot = np.where(cand < n_pred, cand, -1).astype(np.int32)
    desc_now = pool[cand].copy()
    turn = rng.choice(cand.size, 200, replace=False)
    desc_now[turn] = kdesc[rng.integers(0, len(kdesc), turn.size)]
    skip_c = (rng.random(cand.size) < 0.1).astype(np.uint8)
    g = P1 + cand
    take = lambda arr, w: arr.reshape(-1, w)[g]
    return cand, slot, skip_c, desc_now, (take(sc.pos, 3), take(sc.normal, 3), take(sc.min_dist, 1), take(sc.max_dist, 1), desc_now)
