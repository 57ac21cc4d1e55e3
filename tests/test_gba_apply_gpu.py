"""GPU: ccm_gba_apply_map against the numpy checker of test_gba_apply_cpu.py (bit-identical): the three sizes, the smallest shapes that can go wrong, the handle
form against the host form on a BA handle, every CCM_E_ARG case, NaN / Inf, the host mirror on a device against the mirror without one, and two contexts on two
threads."""
import threading

import numpy as np
import pytest

from test_gba_apply_cpu import KEYS, assert_same, bad_arguments, check_flat, ref_pose_of_se3, same_bits

f32 = np.float32


@pytest.fixture(scope="module")
def G():
    from ccm_slam_amd import gba_apply
    return gba_apply


_SCENES = {}


def _scene(G, size):
    """flat arguments and the checker's answer of one of the three sizes, computed once"""
    if size not in _SCENES:
        n_kf, n_pt = G.SIZES[size]
        f = G.flatten(G.make_scene(seed=200 + n_kf, n_kf=n_kf, n_pt=n_pt))
        _SCENES[size] = (f, check_flat(f))
    return _SCENES[size]


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["loop", "agent", "agents4"])
def test_device_matches_the_checker(ctx, G, size):
    f, exp = _scene(G, size)
    assert (f["kf_cam"] < 0).sum() >= 16 and (exp["status"] == 2).sum() > 100
    assert_same(G.apply_map(ctx, f), exp, size)


@pytest.mark.gpu
def test_edge_shapes(ctx, G):
    plain = dict(chains=(), branching=False, vertex_below=False, extra_nonvert=0, n_unreached=0)
    # one origin alone, no points, the per-point pointers NULL
    f = G.flatten(G.make_scene(seed=41, n_kf=1, n_pt=0, n_origins=1, **plain))
    assert f["n_kf"] == 1
    g = dict(f, n_pt=0, pos=None, pt_vert=None, pt_ref=None, null_pos_out=True, null_pt_status=True)
    out = G.apply_map(ctx, g)
    exp = check_flat(f)
    assert same_bits(out["T_new"], exp["T_new"]) and same_bits(out["Twc_new"], exp["Twc_new"])
    # one point of each kind
    for kind in range(3):
        sc = G.make_scene(seed=42 + kind, n_kf=12, n_pt=1, chains=(2,), branching=False, vertex_below=False, extra_nonvert=0, n_unreached=0,
                          vertex_frac=(1.0, 0.0, 0.0)[kind], moved_frac=(0.0, 1.0, 0.0)[kind])
        f = G.flatten(sc)
        exp = check_flat(f)
        assert f["pos"].shape[0] == 1 and exp["status"][0] == (1, 2, 0)[kind]
        assert_same(G.apply_map(ctx, f), exp, f"one point, kind {kind}")
    # a ragged last workgroup of the point kernel
    f = G.flatten(G.make_scene(seed=45, n_kf=30, n_pt=64 * 3 + 5))
    exp = check_flat(f)
    assert set(np.unique(exp["status"])) == {0, 1, 2} and exp["status"][-5:].size == 5
    assert_same(G.apply_map(ctx, f), exp, "ragged")
    # no keyframe that was no vertex: the tree kernel is not launched
    f = G.flatten(G.make_scene(seed=46, n_kf=70, n_pt=100, **plain))
    assert (f["kf_cam"] >= 0).all()
    assert_same(G.apply_map(ctx, f), check_flat(f), "vertices only")
    # a single chain of depth 40
    sc = G.make_scene(seed=47, n_kf=50, n_pt=200, chains=(40,), branching=False, vertex_below=False, extra_nonvert=0, n_unreached=0, moved_frac=0.5, vertex_frac=0.4)
    f = G.flatten(sc)
    depth = np.zeros(f["n_kf"], int)
    for k in range(f["n_kf"]):
        depth[k] = 0 if f["kf_cam"][k] >= 0 else depth[f["kf_parent"][k]] + 1
    assert depth.max() == 40 and (f["kf_cam"] < 0).sum() == 40
    exp = check_flat(f)
    assert (exp["status"] == 2).sum() > 50
    assert_same(G.apply_map(ctx, f), exp, "chain of 40")
    # one level wider than the tree kernel's workgroup (256 lanes), under a single parent, next to deeper levels
    sc = G.make_scene(seed=48, n_kf=360, n_pt=500, wide_level=300, extra_nonvert=0, moved_frac=0.5, vertex_frac=0.4)
    f = G.flatten(sc)
    nonv = f["kf_cam"] < 0
    assert np.bincount(f["kf_parent"][nonv]).max() >= 300
    assert_same(G.apply_map(ctx, f), check_flat(f), "wide level")
    # a vertex below a keyframe that was none keeps its own estimate, and is depth 0 for the one below it
    f = G.flatten(G.make_scene(seed=49, n_kf=12, n_pt=40, chains=(), branching=False, vertex_below=True, extra_nonvert=0, n_unreached=0))
    par, cam = f["kf_parent"], f["kf_cam"]
    v = np.nonzero((cam >= 0) & (par >= 0) & (cam[np.maximum(par, 0)] < 0))[0]
    assert v.size == 1
    out = G.apply_map(ctx, f)
    assert same_bits(out["T_new"][v[0]], ref_pose_of_se3(f["cam_qt"][cam[v[0]]])[0])
    assert_same(out, check_flat(f), "vertex below")


def _ba_scene(G, prob, cam, pts, rng):
    """a walk over the cameras of a BA problem: camera c is keyframe c (a chain from camera 0), three keyframes that were no vertices hang below, the landmarks
    are points and some further points move with a reference keyframe"""
    n_cam, n_lm = int(prob["n_cam"]), int(prob["n_pt"])
    n_kf = n_cam + 3
    kf_parent = np.concatenate([[-1], np.arange(n_cam - 1), [3, n_cam, 7]]).astype(np.int32)
    kf_cam = np.concatenate([np.arange(n_cam), [-1, -1, -1]]).astype(np.int32)
    Tcw = np.concatenate([ref_pose_of_se3(prob["cam_qt"]), ref_pose_of_se3(np.asarray(prob["cam_qt"]).reshape(-1, 7)[[3, 4, 7]])])
    Tcw[n_cam:, 3::4] += f32(0.25)
    extra = 90
    pos = np.concatenate([np.asarray(prob["pt_xyz"], np.float64).reshape(-1, 3), rng.normal(0, 3, (extra, 3))]).astype(f32)
    pt_vert = np.concatenate([np.arange(n_lm), np.full(extra, -1)]).astype(np.int32)
    pt_ref = np.concatenate([rng.integers(0, n_kf, n_lm), rng.integers(-1, n_kf, extra)]).astype(np.int32)
    return dict(n_kf=n_kf, kf_parent=kf_parent, kf_cam=kf_cam, Tcw_old=Tcw, Twc_old=G.inverse_pose(Tcw), pos=pos, pt_vert=pt_vert, pt_ref=pt_ref,
                cam_qt=cam, pt_xyz=pts)


@pytest.mark.gpu
def test_handle_form_gives_the_bits_of_the_host_form(ctx, G):
    from ccm_slam_amd import optimizer, synth
    from ccm_slam_amd._lib import CcmError, Context
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=20, n_points=300, seed=4, n_fixed=2)
    ba = optimizer.BAHandle(ctx, prob)
    try:
        ba.run(2)
        cam, pts, _, _ = ba.download()
        assert not same_bits(cam, np.ascontiguousarray(prob["cam_qt"], np.float64)) and not same_bits(pts, np.ascontiguousarray(prob["pt_xyz"], np.float64))
        f = _ba_scene(G, prob, cam, pts, np.random.default_rng(3))
        exp = check_flat(f)
        assert set(np.unique(exp["status"])) == {0, 1, 2}
        host_form = G.apply_map(ctx, f)
        assert_same(host_form, exp, "host form")
        h = dict(f, cam_qt=None, pt_xyz=None)
        assert_same(G.apply_map(ctx, h, ba=ba), host_form, "handle form")
        assert_same(G.apply_map(ctx, dict(h, n_pt=0), ba=ba), dict(exp, pos=exp["pos"][:0], status=exp["status"][:0]), "handle form, no points")
        cam2, pts2, _, _ = ba.download()                        # the handle's own state is unchanged
        assert same_bits(cam2, cam) and same_bits(pts2, pts)
        # both forms at once; a handle of another context; indices beyond the handle's own counts
        with pytest.raises(CcmError):
            G.apply_map(ctx, f, ba=ba)
        with pytest.raises(CcmError):
            G.apply_map(ctx, dict(h, pt_xyz=pts), ba=ba)
        other = Context(0)
        try:
            with pytest.raises(CcmError):
                G.apply_map(other, h, ba=ba)
        finally:
            other.close()
        for key, val in (("kf_cam", int(prob["n_cam"])), ("pt_vert", int(prob["n_pt"]))):
            a = f[key].copy(); a[0] = val
            with pytest.raises(CcmError):
                G.apply_map(ctx, dict(h, **{key: a}), ba=ba)
        assert_same(G.apply_map(ctx, h, ba=ba), host_form, "handle form after the refused calls")
    finally:
        ba.close()


@pytest.mark.gpu
def test_refused_arguments_and_nan_inf(ctx, G):
    from ccm_slam_amd._lib import CcmError
    f = G.flatten(G.make_scene(seed=8, n_kf=40, n_pt=50))
    exp = check_flat(f)
    for name, g in bad_arguments(G, f):
        with pytest.raises(CcmError):
            G.apply_map(ctx, g)
            pytest.fail(name + " was accepted")
    assert_same(G.apply_map(ctx, f), exp, "after the refused calls")
    pos = f["pos"].copy(); pos[0, 0] = np.nan; pos[1, 1] = np.inf
    cq = f["cam_qt"].copy(); cq[f["kf_cam"][0], 4] = np.nan; cq[f["kf_cam"][1], 0] = np.inf
    g = dict(f, pos=pos, cam_qt=cq)
    with np.errstate(invalid="ignore"):
        exp = check_flat(g)
    out = G.apply_map(ctx, g)
    assert np.isnan(out["T_new"]).any() and np.isnan(out["pos"]).any()
    for k in KEYS:   # NaN payloads are not part of the contract: the same places are NaN, everything else has the same bits
        a, b = np.asarray(out[k]), np.asarray(exp[k])
        if a.dtype == np.uint8:
            assert np.array_equal(a, b)
            continue
        assert np.array_equal(np.isnan(a), np.isnan(b)) and same_bits(np.where(np.isnan(a), f32(0), a), np.where(np.isnan(b), f32(0), b)), k


@pytest.mark.gpu
def test_host_mirror_with_a_device_against_the_mirror_without_one(G):
    sc = G.make_scene(seed=12, n_kf=80, n_pt=900)
    a, b = G.MapUpdate(sc, device=0), G.MapUpdate(sc)
    try:
        ra, rb = a.results(), b.results()
        assert a.reached_twice == b.reached_twice == 0 and a.stale_references == b.stale_references > 0 and a.n_reached == b.n_reached == 76
        assert np.array_equal(ra["order"], rb["order"]) and np.array_equal(ra["kf_parent"], rb["kf_parent"])
        assert_same(ra, rb, "mirror")
        assert_same(ra, check_flat(G.flatten(sc)), "mirror against the checker")
    finally:
        a.close(); b.close()


@pytest.mark.gpu
def test_two_contexts_on_two_threads(G):
    from ccm_slam_amd._lib import Context
    jobs = [_scene(G, "loop"), _scene(G, "agent")]
    errs = []

    def work(i):
        try:
            c = Context(0)
            try:
                for _ in range(4):
                    assert_same(G.apply_map(c, jobs[i][0]), jobs[i][1], f"thread {i}")
            finally:
                c.close()
        except BaseException as e:   # noqa: BLE001 - handed to the main thread
            errs.append(e)
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
