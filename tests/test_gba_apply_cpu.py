"""CPU: the map update that follows a global BA (ccm_slam_amd/csrc/gba_apply_math.h through the host evaluator).  No device is touched.

 * a literal sequential replay of the reference's walk (Map.cpp:1441-1568: a list, pop_front / push_back, poses, mTcwBefGBA and tags mutated as it goes)
   against the flat evaluator and the host mirror, bit for bit;
 * an independent numpy checker (one ufunc per operation, so nothing can fuse), bit-identical to the header at the three sizes;
 * known answers on exactly representable inputs; order independence inside a level; the refused orders; the twice-reached keyframe and the tagged but
   unreached reference keyframe.
All comparisons are for identical bits (the known answers: for equal values)."""
import numpy as np
import pytest

f32, f64 = np.float32, np.float64
KEYS = ("T_new", "Twc_new", "pos", "status")


@pytest.fixture(scope="module")
def G():
    from ccm_slam_amd import gba_apply
    return gba_apply


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def assert_same(got, exp, tag=""):
    for k in KEYS:
        g = np.asarray(got[k]).reshape(np.asarray(exp[k]).shape)
        assert same_bits(g, np.asarray(exp[k])), (tag, k, int((g != exp[k]).sum()) if g.size else 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the numpy checker
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ref_pose_of_se3(qt):
    """Converter::toCvMat(SE3Quat), rows 0..2, for (n, 7) f64: Eigen's toRotationMatrix on the quaternion as it is"""
    qt = np.asarray(qt, f64).reshape(-1, 7)
    qx, qy, qz, qw = qt[:, 0], qt[:, 1], qt[:, 2], qt[:, 3]
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    R = [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]
    T = np.zeros((qt.shape[0], 12), f32)
    for r in range(3):
        for c in range(3):
            T[:, 4 * r + c] = R[3 * r + c].astype(f32)
        T[:, 4 * r + 3] = qt[:, 4 + r].astype(f32)
    return T


def ref_gemm44(A, B):
    """rows 0..2 of A * B for (n, 12) f32 operands with last rows 0 0 0 1: f32 accumulator, the four products added left to right"""
    A = np.asarray(A, f32).reshape(-1, 12); B = np.asarray(B, f32).reshape(-1, 12)
    out = np.zeros((max(A.shape[0], B.shape[0]), 12), f32)
    for r in range(3):
        for c in range(4):
            t = A[:, 4 * r] * B[:, c]
            t = t + A[:, 4 * r + 1] * B[:, 4 + c]
            t = t + A[:, 4 * r + 2] * B[:, 8 + c]
            t = t + A[:, 4 * r + 3] * f32(1.0 if c == 3 else 0.0)
            out[:, 4 * r + c] = t
    return out


def ref_twc(T):
    """rows 0..2 of the Twc of KeyFrame::SetPose: Rwc = Rcw.t(), Ow = -Rwc * tcw as one gemm with alpha = -1"""
    T = np.asarray(T, f32).reshape(-1, 12)
    W = np.zeros_like(T)
    for r in range(3):
        t = T[:, r] * T[:, 3]
        t = t + T[:, 4 + r] * T[:, 7]
        t = t + T[:, 8 + r] * T[:, 11]
        W[:, 4 * r + 3] = (t.astype(f64) * -1.0 + 0.0).astype(f32)
        W[:, 4 * r] = T[:, r]; W[:, 4 * r + 1] = T[:, 4 + r]; W[:, 4 * r + 2] = T[:, 8 + r]
    return W


def ref_gemm_rt(M, x):
    """A * x + c as one cv::gemm(A, x, 1, c, 1) per row of M (n, 12) and x (n, 3)"""
    out = np.zeros(x.shape, f32)
    for r in range(3):
        t = M[:, 4 * r] * x[:, 0]
        t = t + M[:, 4 * r + 1] * x[:, 1]
        t = t + M[:, 4 * r + 2] * x[:, 2]
        out[:, r] = (t.astype(f64) * 1.0 + M[:, 4 * r + 3].astype(f64) * 1.0).astype(f32)
    return out


def check_flat(f):
    """the outputs of ccm_gba_apply_map for the arguments of flatten, computed with numpy alone"""
    par = np.asarray(f["kf_parent"]); cam = np.asarray(f["kf_cam"]); n_kf = par.size
    Tcw = np.asarray(f["Tcw_old"], f32).reshape(-1, 12); Twc = np.asarray(f["Twc_old"], f32).reshape(-1, 12)
    T = np.zeros((n_kf, 12), f32)
    v = cam >= 0
    T[v] = ref_pose_of_se3(np.asarray(f["cam_qt"], f64).reshape(-1, 7)[cam[v]])
    depth = np.zeros(n_kf, np.int64)
    for k in np.nonzero(~v)[0]:
        depth[k] = depth[par[k]] + 1
    for d in range(1, int(depth.max()) + 1 if n_kf else 0):   # a level at a time: every parent is finished
        ks = np.nonzero(depth == d)[0]
        T[ks] = ref_gemm44(ref_gemm44(Tcw[ks], Twc[par[ks]]), T[par[ks]])
    W = ref_twc(T)
    pos = np.asarray(f["pos"], f32).reshape(-1, 3) if f.get("pos") is not None else np.zeros((0, 3), f32)
    n_pt = int(f.get("n_pt", pos.shape[0])); pos = pos[:n_pt]
    out = pos.copy(); status = np.zeros(n_pt, np.uint8)
    if n_pt:
        vert = np.asarray(f["pt_vert"])[:n_pt]; ref = np.asarray(f["pt_ref"])[:n_pt]
        a = vert >= 0
        out[a] = np.asarray(f["pt_xyz"], f64).reshape(-1, 3)[vert[a]].astype(f32); status[a] = 1
        m = ~a & (ref >= 0)
        out[m] = ref_gemm_rt(W[ref[m]], ref_gemm_rt(Tcw[ref[m]], pos[m])); status[m] = 2
    return dict(T_new=T, Twc_new=W, pos=out, status=status)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the literal replay
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _mat4(T12):
    return np.concatenate([np.asarray(T12, f32).reshape(3, 4), np.array([[0, 0, 0, 1]], f32)], 0)


def _gemm(A, B, alpha=1.0, Cm=None):
    """cv::gemm's small-matrix path on f32 matrices with inner dimension 3 or 4, element by element"""
    out = np.zeros((A.shape[0], B.shape[1]), f32)
    for r in range(A.shape[0]):
        for c in range(B.shape[1]):
            t = f32(A[r, 0] * B[0, c])
            for k in range(1, A.shape[1]):
                t = f32(t + f32(A[r, k] * B[k, c]))
            out[r, c] = t if (Cm is None and alpha == 1.0) else f32(f64(t) * alpha + (f64(Cm[r, c]) * 1.0 if Cm is not None else 0.0))
    return out


class _KF:
    def __init__(self, Tcw, Twc):
        self.Tcw = _mat4(Tcw); self.Twc = _mat4(Twc); self.TcwGBA = None; self.TcwBefGBA = None; self.tag = 0; self.childs = []; self.corrected = False

    def set_pose(self, T):
        self.Tcw = T.copy()
        Rwc = self.Tcw[:3, :3].T
        Ow = _gemm(Rwc, self.Tcw[:3, 3:4], alpha=-1.0)
        self.Twc = np.eye(4, dtype=f32)
        self.Twc[:3, :3] = Rwc; self.Twc[:3, 3:4] = Ow


def replay(sc, loop_tag=7):
    """Optimizer.cpp:803-857 and Map.cpp:1441-1568 on a scene, object by object.  Returns per keyframe id the pose and inverse (None where the walk did not
    come), the positions and what happened to every point."""
    n = int(sc["n_kf"])
    kfs = [_KF(sc["Tcw"][i], sc["Twc"][i]) for i in range(n)]
    for i in range(n):
        kfs[i].childs = [kfs[c] for c in sc["child_kf"][sc["child_off"][i]:sc["child_off"][i + 1]]]
        if sc["kf_cam"][i] >= 0:   # recovery: the vertices
            kfs[i].TcwGBA = _mat4(ref_pose_of_se3(sc["cam_qt"][sc["kf_cam"][i]])[0]); kfs[i].tag = loop_tag
    lst = [kfs[o] for o in sc["origins"]]
    while lst:
        kf = lst[0]
        Twc = kf.Twc
        for child in kf.childs:
            if child.tag != loop_tag:
                Tchildc = _gemm(child.Tcw, Twc)
                child.TcwGBA = _gemm(Tchildc, kf.TcwGBA)
                child.tag = loop_tag
            lst.append(child)
        kf.TcwBefGBA = kf.Tcw
        kf.set_pose(kf.TcwGBA)
        kf.corrected = True
        lst.pop(0)
    pos = np.asarray(sc["pos"], f32).copy(); status = np.zeros(pos.shape[0], np.uint8)
    for i in range(pos.shape[0]):
        if sc["pt_vert"][i] >= 0:
            pos[i] = np.asarray(sc["pt_xyz"][sc["pt_vert"][i]], f64).astype(f32); status[i] = 1
            continue
        r = sc["pt_ref_kf"][i]
        if r < 0 or kfs[r].tag != loop_tag:
            continue
        if kfs[r].TcwBefGBA is None:   # tagged, never walked: the reference reads whatever an earlier run left there
            continue
        ref = kfs[r]
        Xc = _gemm(ref.TcwBefGBA[:3, :3], pos[i].reshape(3, 1), Cm=ref.TcwBefGBA[:3, 3:4])
        pos[i] = _gemm(ref.Twc[:3, :3], Xc, Cm=ref.Twc[:3, 3:4]).reshape(3); status[i] = 2
    return kfs, pos, status


def _by_id(f, out, n):
    """flat outputs scattered to keyframe ids"""
    T = np.full((n, 12), np.nan, f32); W = np.full((n, 12), np.nan, f32)
    T[f["order"]] = out["T_new"]; W[f["order"]] = out["Twc_new"]
    return T, W


def test_literal_replay_of_the_reference_walk(G):
    sc = G.make_scene(seed=5, n_kf=40, n_pt=400, extra_nonvert=2)
    f = G.flatten(sc)
    # the scene holds what it must: two origins, chains of depth 1, 2 and 5, a branching subtree, a vertex under a non-vertex, every point kind
    assert sc["origins"].size == 2 and f["n_twice"] == 0
    par, cam = f["kf_parent"], f["kf_cam"]
    depth = np.zeros(par.size, int)
    for k in range(par.size):
        depth[k] = 0 if cam[k] >= 0 else depth[par[k]] + 1
    at = np.full(sc["n_kf"], -1); at[f["order"]] = np.arange(par.size)
    assert sorted(depth[at[sc["chain_ends"]]]) == [1, 2, 5]
    nonv = cam < 0
    kids = np.bincount(par[(par >= 0) & nonv], minlength=par.size)
    assert ((kids >= 2) & nonv).sum() >= 2                                    # non-vertices with several non-vertex children
    assert ((cam >= 0) & (par >= 0) & nonv[np.maximum(par, 0)]).any()         # a vertex under a non-vertex ...
    assert (nonv & (par >= 0) & (cam[np.maximum(par, 0)] >= 0) & nonv[np.maximum(par[np.maximum(par, 0)], 0)]).any()   # ... with a non-vertex below it
    assert all((sc["pt_kind"] == k).sum() >= 1 for k in range(5)) and f["n_stale"] == (sc["pt_kind"] == G.PT_REF_UNREACHED).sum() > 0
    kfs, pos, status = replay(sc)
    out = G.apply_map_host(f)
    T, W = _by_id(f, out, sc["n_kf"])
    for i, kf in enumerate(kfs):
        if not kf.corrected:
            assert at[i] < 0
            continue
        assert same_bits(kf.Tcw[:3].reshape(12), T[i]) and same_bits(kf.Twc[:3].reshape(12), W[i]), i
    assert same_bits(pos, out["pos"]) and np.array_equal(status, out["status"])
    assert set(np.unique(status)) == {0, 1, 2}
    assert (status[sc["pt_kind"] >= G.PT_NO_REF] == 0).all() and (status[sc["pt_kind"] == G.PT_MOVED] == 2).all()
    # the host mirror flattens the same walk and gives the same bits
    m = G.MapUpdate(sc)
    res = m.results()
    assert m.reached_twice == 0 and m.stale_references == f["n_stale"] and m.n_reached == f["n_kf"]
    assert np.array_equal(res["order"], f["order"]) and np.array_equal(res["kf_parent"], f["kf_parent"])
    assert_same(res, out, "mirror")
    assert_same(out, check_flat(f), "checker")
    m.close()


@pytest.mark.parametrize("size", ["loop", "agent", "agents4"])
def test_header_matches_the_numpy_checker(G, size):
    n_kf, n_pt = G.SIZES[size]
    f = G.flatten(G.make_scene(seed=200 + n_kf, n_kf=n_kf, n_pt=n_pt))
    assert f["n_kf"] == n_kf - 4 and (f["kf_cam"] < 0).sum() >= 16
    exp = check_flat(f)
    assert_same(G.apply_map_host(f), exp, size)
    assert (exp["status"] == 1).sum() > 0.8 * n_pt and (exp["status"] == 2).sum() > 0.05 * n_pt


# ---------------------------------------------------------------------------------------------------------------------------------------------
# known answers
# ---------------------------------------------------------------------------------------------------------------------------------------------
_HALF = {(1, 1, 1): (0, 0, 0, 1), (1, -1, -1): (1, 0, 0, 0), (-1, 1, -1): (0, 1, 0, 0), (-1, -1, 1): (0, 0, 1, 0)}   # diag(R) -> exact quaternion


def _quarter(rng):
    """a rotation of the cube: a signed permutation matrix with determinant +1"""
    while True:
        R = np.zeros((3, 3)); R[np.arange(3), rng.permutation(3)] = rng.choice([-1.0, 1.0], 3)
        if np.linalg.det(R) > 0:
            return R


def _integer_scene(G, seed=3):
    """parent chain: origin V0 (vertex) -> N1 -> N2 -> N3 (no vertices), V0 -> V4 (vertex) -> N5; half turns and integer translations for the vertices (their
    quaternions are exact), rotations of the cube for the others; integer points on N1, N3, N5 and V4"""
    rng = np.random.default_rng(seed)
    parent = [-1, 0, 1, 2, 0, 4]; vertex = [True, False, False, False, True, False]
    n = len(parent)
    Tcw = np.zeros((n, 12), f32); cam_qt = np.zeros((2, 7)); kf_cam = np.full(n, -1, np.int32)
    diags = list(_HALF)
    for i in range(n):
        R = np.diag(np.array(diags[1 + i % 3], float)) if vertex[i] else _quarter(rng)
        t = rng.integers(-9, 10, 3).astype(float)
        Tcw[i] = np.concatenate([R, t[:, None]], 1).reshape(12)
        if vertex[i]:
            kf_cam[i] = 1 - i // 4
            cam_qt[kf_cam[i]] = np.concatenate([_HALF[diags[1 + i % 3]], t])
    child = [[c for c in range(n) if parent[c] == p] for p in range(n)]
    ref = np.array([1, 3, 5, 4, 3, 1], np.int32)
    pos = rng.integers(-20, 21, (ref.size, 3)).astype(f32)
    return dict(n_kf=n, origins=np.array([0], np.int32), child_off=np.cumsum([0] + [len(c) for c in child]).astype(np.int32),
                child_kf=np.array(sum(child, []), np.int32), kf_cam=kf_cam, Tcw=Tcw, Twc=G.inverse_pose(Tcw), cam_qt=cam_qt, pt_xyz=np.zeros((0, 3)), pos=pos,
                pt_vert=np.full(ref.size, -1, np.int32), pt_ref_kf=ref)


def test_known_answer_old_poses_returned_nothing_moves(G):
    sc = _integer_scene(G)
    f = G.flatten(sc)
    out = G.apply_map_host(f)
    assert np.array_equal(out["T_new"], f["Tcw_old"]) and np.array_equal(out["Twc_new"], f["Twc_old"])     # values: -0 and +0 are the same place
    assert np.array_equal(out["pos"], sc["pos"]) and (out["status"] == 2).all()


def test_known_answer_integer_translation_of_the_parent(G):
    sc = _integer_scene(G)
    d = np.array([3.0, -7.0, 11.0])
    moved = dict(sc, cam_qt=sc["cam_qt"].copy())
    c0 = sc["kf_cam"][0]
    R0 = sc["Tcw"][0].reshape(3, 4)[:, :3].astype(float)
    moved["cam_qt"][c0, 4:] = sc["cam_qt"][c0, 4:] - R0 @ d          # the origin's centre moves by d; the other vertex stays
    f = G.flatten(moved)
    out = G.apply_map_host(f)
    T, W = _by_id(f, out, sc["n_kf"])
    old_c = sc["Twc"][:, 3::4]
    for i, shift in enumerate([d, d, d, d, 0 * d, 0 * d]):             # N1..N3 hang below the origin, N5 below the vertex that stayed
        assert np.array_equal(W[i, 3::4], (old_c[i] + shift).astype(f32)), i
        assert np.array_equal(T[i].reshape(3, 4)[:, :3], sc["Tcw"][i].reshape(3, 4)[:, :3]), i
    shift_pt = np.array([d, d, 0 * d, 0 * d, d, d])
    assert np.array_equal(out["pos"], (sc["pos"] + shift_pt).astype(f32))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the order
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_children_of_a_level_in_any_order(G):
    sc = G.make_scene(seed=6, n_kf=60, n_pt=300, wide_level=7)
    rev = dict(sc, child_kf=np.concatenate([sc["child_kf"][a:b][::-1] for a, b in zip(sc["child_off"][:-1], sc["child_off"][1:])]).astype(np.int32),
               origins=sc["origins"][::-1].copy())
    f, g = G.flatten(sc), G.flatten(rev)
    assert not np.array_equal(f["order"], g["order"]) and sorted(f["order"]) == sorted(g["order"])
    a, b = G.apply_map_host(f), G.apply_map_host(g)
    Ta, Wa = _by_id(f, a, sc["n_kf"]); Tb, Wb = _by_id(g, b, sc["n_kf"])
    assert same_bits(Ta, Tb) and same_bits(Wa, Wb) and same_bits(a["pos"], b["pos"]) and np.array_equal(a["status"], b["status"])


def bad_arguments(G, f):
    """(name, arguments) of every refused call, for the host evaluator and the device entry alike"""
    n = f["n_kf"]
    nonv = int(np.nonzero(f["kf_cam"] < 0)[0][0])

    def put(key, idx, val):
        a = np.array(f[key]).copy(); a[idx] = val
        return dict(f, **{key: a})
    cases = [("n_kf < 1", dict(f, n_kf=0)), ("n_pt < 0", dict(f, n_pt=-1)),
             ("a parent at its child", put("kf_parent", 3, 3)), ("a parent behind its child", put("kf_parent", 3, n - 1)), ("a parent < -1", put("kf_parent", 3, -2)),
             ("camera out of range", put("kf_cam", 0, f["cam_qt"].shape[0])), ("landmark out of range", put("pt_vert", 0, f["pt_xyz"].shape[0])),
             ("reference out of range", put("pt_ref", 1, n)), ("an origin that was no vertex", put("kf_parent", nonv, -1)),
             ("neither state form", dict(f, cam_qt=None, pt_xyz=None, n_cam=f["cam_qt"].shape[0], n_lm=f["pt_xyz"].shape[0])),
             ("landmarks missing", dict(f, pt_xyz=None, n_lm=f["pt_xyz"].shape[0]))]
    cases += [("null " + k, dict(f, **{k: None}, n_kf=n, n_pt=f["pos"].shape[0])) for k in ("kf_parent", "kf_cam", "Tcw_old", "Twc_old", "pos", "pt_vert", "pt_ref")]
    cases += [("null " + k, dict(f, **{"null_" + k: True})) for k in ("T_new", "Twc_new", "pos_out", "pt_status")]
    return cases


def test_refused_orders_and_arguments(G):
    from ccm_slam_amd._lib import CcmError
    f = G.flatten(G.make_scene(seed=8, n_kf=40, n_pt=50))
    G.apply_map_host(f)
    for name, g in bad_arguments(G, f):
        with pytest.raises(CcmError):
            G.apply_map_host(g)
            pytest.fail(name + " was accepted")
    # no points at all, the per-point pointers NULL
    g = dict(f, n_pt=0, pos=None, pt_vert=None, pt_ref=None, null_pos_out=True, null_pt_status=True)
    out = G.apply_map_host(g)
    assert same_bits(out["T_new"], check_flat(f)["T_new"]) and out["pos"].shape[0] == 0


def test_twice_reached_keyframe_and_unreached_tagged_reference(G):
    sc = G.make_scene(seed=9, n_kf=40, n_pt=200)
    f = G.flatten(sc)
    m = G.MapUpdate(sc)
    res = m.results()
    stale = sc["pt_kind"] == G.PT_REF_UNREACHED
    assert m.reached_twice == 0 and m.stale_references == stale.sum() == f["n_stale"] > 0
    assert (res["status"][stale] == 0).all() and same_bits(res["pos"][stale], sc["pos"][stale])
    assert (sc["kf_cam"][sc["unreached_vertex"]] >= 0).all() and not np.isin(sc["unreached_vertex"], f["order"]).any()
    m.close()
    # one keyframe in two child sets: the reference would visit it twice
    twice = int(f["order"][-1]); other = int(f["order"][1])
    off, ch = sc["child_off"], sc["child_kf"]
    ch2 = np.insert(ch, off[other + 1], twice).astype(np.int32)
    off2 = off.copy(); off2[other + 1:] += 1
    sc2 = dict(sc, child_off=off2, child_kf=ch2)
    assert twice not in ch[off[other]:off[other + 1]]
    assert G.flatten(sc2)["n_twice"] == 1
    m = G.MapUpdate(sc2)
    assert m.reached_twice == 1
    res = m.results()
    assert (res["status"] == 0).all() and same_bits(res["pos"], sc["pos"])       # nothing was evaluated: the caller takes the sequential walk
    m.close()


def test_nan_and_inf_propagate(G):
    f = G.flatten(G.make_scene(seed=10, n_kf=40, n_pt=64))
    pos = f["pos"].copy(); pos[0, 0] = np.nan; pos[1, 1] = np.inf
    cq = f["cam_qt"].copy(); cq[f["kf_cam"][0], 4] = np.nan
    g = dict(f, pos=pos, cam_qt=cq)
    with np.errstate(invalid="ignore"):
        exp = check_flat(g)
    out = G.apply_map_host(g)
    assert np.isnan(out["T_new"][0, 3]) and np.isnan(exp["T_new"][0, 3])
    for k in KEYS:   # NaN payloads are not part of the contract: the same places are NaN, everything else has the same bits
        a, b = np.asarray(out[k]), np.asarray(exp[k])
        if a.dtype == np.uint8:
            assert np.array_equal(a, b)
            continue
        assert np.array_equal(np.isnan(a), np.isnan(b)) and same_bits(np.where(np.isnan(a), f32(0), a), np.where(np.isnan(b), f32(0), b)), k
