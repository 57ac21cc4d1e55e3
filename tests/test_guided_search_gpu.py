"""ccm_frame_guided_search, the mirror's SearchByProjection(Frame&, kfptr, sAlreadyFound, th, ORBdist) with a grid and cslam::RelocalizationRefine on the device,
against the host evaluator, the host mirror and tests/guided_search_cases.py's replay.  Every comparison is equality of integers or of float bits."""
import ctypes as C

import numpy as np
import pytest

import guided_search_cases as gc
from ccm_slam_amd import optimizer, reloc
from ccm_slam_amd._lib import CcmError, _p, host, lib
from ccm_slam_amd.frame import FrameGrid
from guided_search_cases import assert_evaluation, host_eval, host_mirror, kf_of, pose_of, skip_of

pytestmark = pytest.mark.gpu
GATE_TPB = 256          # the gate kernel's workgroup
CCM_E_ARG = -1


def grid_of(ctx, frame):
    g = FrameGrid(ctx, frame["K"], np.zeros(0, np.float32), gc.W, gc.H)
    g.set_keypoints(frame["kps"], frame["desc"])
    assert np.array_equal(g.bounds, frame["bounds"])
    return g


def device_eval(ctx, frame, T, kf, th, **kw):
    g = grid_of(ctx, frame)
    try:
        return reloc.guided_search(g, pose_of(T), kf["pos"], kf["dmin"], kf["dmax"], kf["desc"], skip_of(kf), th, **kw)
    finally:
        g.close()


def head(kf, P):
    return {k: (None if v is None else v[:P]) for k, v in kf.items()}


@pytest.fixture(scope="module")
def scene():
    frame, T, kf = gc.random_scene(1, P=GATE_TPB + 40, n_clutter=150)
    assert 250 <= len(frame["kps"]) <= 450
    return frame, T, kf


@pytest.mark.parametrize("th", [3.0, 10.0])
def test_device_equals_host_evaluator(ctx, scene, th):
    frame, T, kf = scene
    feats = {n: dict(frame, kps=frame["kps"][:n], desc=frame["desc"][:n], mp=frame["mp"][:n]) for n in (0, 1, len(frame["kps"]))}
    for P in (0, 1, 7, 8, 9, GATE_TPB - 1, GATE_TPB, GATE_TPB + 1, len(kf["live"])):
        k = head(kf, P)
        for n, f in feats.items():
            if n != len(frame["kps"]) and P not in (0, 9, len(kf["live"])):
                continue
            want = host_eval(f, T, k, th)
            assert_evaluation(device_eval(ctx, f, T, k, th), want, (P, n, th))
    full = host_eval(frame, T, kf, th)
    assert set(full["status"]) == {0, 1, 2, 3} and full["n_cand"] > 100


def test_no_skip_array_searches_every_slot(ctx, scene):
    frame, T, kf = scene
    g = grid_of(ctx, frame)
    got = reloc.guided_search(g, pose_of(T), kf["pos"], kf["dmin"], kf["dmax"], kf["desc"], None, 10.0)
    g.close()
    want = reloc.guided_search_host(frame["kps"], frame["desc"], frame["bounds"], frame["K"], pose_of(T), kf["pos"], kf["dmin"], kf["dmax"], kf["desc"], None, 10.0)
    assert_evaluation(got, want, "no skip")
    assert not np.any(got["status"] == gc.SKIPPED)


@pytest.mark.parametrize("case", gc.edge_cases(), ids=lambda c: c[0])
def test_planted_edge_on_the_device(ctx, case):
    name, frame, T, kf, th, orb_dist, ori, expect = case
    r = gc.replay(frame, T, kf, th, orb_dist, ori)
    expect(r)
    assert_evaluation(device_eval(ctx, frame, T, kf, th), r, name)
    n, mp = reloc.search_by_projection_kf(ctx, frame["K"], gc.W, gc.H, frame["kps"], frame["desc"], pose_of(T), kf_of(kf), kf["found"], th, orb_dist, ori, frame["mp"])
    assert n == r["nmatches"] and np.array_equal(mp, r["mp"])


def test_capacity(ctx, scene):
    frame, T, kf = scene
    want = host_eval(frame, T, kf, 10.0)
    total = want["n_cand"]
    sized = device_eval(ctx, frame, T, kf, 10.0, cap=0)
    assert sized["n_cand"] == total and np.array_equal(sized["off"], want["off"]) and np.array_equal(sized["status"], want["status"])
    assert_evaluation(device_eval(ctx, frame, T, kf, 10.0, cap=total), want, "exact capacity")
    with pytest.raises(CcmError) as e:
        device_eval(ctx, frame, T, kf, 10.0, cap=total - 1)
    assert e.value.rc == CCM_E_ARG and e.value.n_cand == total
    assert_evaluation(device_eval(ctx, frame, T, kf, 10.0, cap=10 ** 12), want, "a capacity beyond P * N")


def test_bad_arguments(ctx, scene):
    frame, T, kf = scene
    g = grid_of(ctx, frame)
    P = 9
    pos, dmin, dmax, desc = (np.ascontiguousarray(kf[k][:P]) for k in ("pos", "dmin", "dmax", "desc"))
    st, u, v, lv, off = np.zeros(P, np.uint8), np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.int32), np.zeros(P + 1, np.int32)
    idx, dist, n = np.zeros(4096, np.int32), np.zeros(4096, np.uint16), C.c_int64(0)
    good = dict(f=g._h, pose=pose_of(T), P=P, pos=pos, dmin=dmin, dmax=dmax, desc=desc, th=10.0, st=st, u=u, v=v, lv=lv, off=off, idx=idx, dist=dist, cap=4096, n=C.byref(n))

    def call(**kw):
        a = dict(good, **kw)
        p = lambda x: _p(x) if isinstance(x, np.ndarray) else x
        return lib().ccm_frame_guided_search(a["f"], C.byref(a["pose"]) if a["pose"] is not None else None, a["P"], p(a["pos"]), p(a["dmin"]), p(a["dmax"]), p(a["desc"]), None,
                                             C.c_float(a["th"]), p(a["st"]), p(a["u"]), p(a["v"]), p(a["lv"]), p(a["off"]), p(a["idx"]), p(a["dist"]), C.c_int64(a["cap"]), a["n"])
    assert call() == 0
    for name in ("pose", "pos", "dmin", "dmax", "desc", "st", "u", "v", "lv", "off", "idx", "dist", "n"):
        assert call(**{name: None}) == CCM_E_ARG, name
    assert call(f=None) == CCM_E_ARG
    assert call(P=-1) == CCM_E_ARG and call(cap=-1) == CCM_E_ARG
    for n_levels in (0, -3, 17):
        assert call(pose=reloc.guided_pose(T, gc.LOG_SF, gc.SF, n_levels)) == CCM_E_ARG
    for th in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert call(th=th) == CCM_E_ARG
    assert call(th=0.0) == 0 and n.value == 0
    assert call(P=0, pos=None, dmin=None, dmax=None, desc=None, st=None, u=None, v=None, lv=None) == 0
    n.value = -1
    assert call(cap=1) == CCM_E_ARG and n.value > 1
    g.close()


@pytest.mark.parametrize("ori", [True, False])
def test_mirror_with_a_grid_equals_the_host_mirror(ctx, scene, ori):
    frame, T, kf = scene
    for th, orb_dist in ((10.0, 100), (3.0, 64)):
        want_n, want_mp = host_mirror(frame, T, kf, th, orb_dist, ori)
        n, mp = reloc.search_by_projection_kf(ctx, frame["K"], gc.W, gc.H, frame["kps"], frame["desc"], pose_of(T), kf_of(kf), kf["found"], th, orb_dist, ori, frame["mp"])
        assert n == want_n and np.array_equal(mp, want_mp)
        r = gc.replay(frame, T, kf, th, orb_dist, ori)
        assert n == r["nmatches"] and np.array_equal(mp, r["mp"])
    with pytest.raises(CcmError):
        reloc.search_by_projection_kf(ctx, frame["K"], gc.W, gc.H, frame["kps"], frame["desc"], pose_of(T), kf_of(kf), kf["found"], 10.0, 256, ori, frame["mp"])


@pytest.mark.parametrize("ori", [True, False])
def test_drop_in_form_on_the_callers_lists(ctx, scene, ori):
    """what shim/ORBmatcher_hip.cpp calls: the lists are the caller's own (here the replay's), the distances one ccm_hamming_csr launch, then the sequential pass"""
    frame, T, kf = scene
    for th, orb_dist in ((10.0, 100), (3.0, 64)):
        r = gc.replay(frame, T, kf, th, orb_dist, ori)
        n, mp = reloc.search_by_projection_kf_candidates(ctx, frame["desc"], frame["kps"]["angle"], kf["desc"], kf["angle"], r["off"], r["idx"], orb_dist, ori, frame["mp"])
        assert n == r["nmatches"] and np.array_equal(mp, r["mp"])
    with pytest.raises(CcmError):
        reloc.search_by_projection_kf_candidates(ctx, frame["desc"], frame["kps"]["angle"], kf["desc"], kf["angle"], r["off"], r["idx"] + 10 ** 6, 100, ori, frame["mp"])


# ---- the refine chain against a composition of the replay and the pose-optimisation wrapper -------------------------------------------------------------------
def compose_refine(ctx, sc):
    """The chain's steps, written from their specification, on the replay (the search) and optimizer.pose_optimization (parent code with its own tests)."""
    h = host()
    frame, kf, N = sc["frame"], dict(sc["kf"]), len(sc["frame"]["kps"])
    kps = frame["kps"]
    mp = np.where(sc["inliers"] != 0, sc["matches_f"], -1).astype(np.int32)
    found = np.zeros(len(kf["live"]), np.uint8)
    found[mp[mp >= 0]] = 1
    T = np.asarray(sc["T0"], np.float32).copy().reshape(16)
    T[12:] = (0, 0, 0, 1)
    outlier = np.zeros(N, bool)
    trace = [-1] * 5

    def optimise():
        nonlocal T
        js = np.nonzero(mp >= 0)[0]
        outlier[js] = False
        if js.size < 3:
            return 0
        qt = np.zeros(7)
        h.ccmh_to_se3quat(_p(T), _p(qt))
        obs = np.stack([kps["x"][js], kps["y"][js]], 1).astype(np.float64)
        cam, outl, ninl = optimizer.pose_optimization(ctx, qt, kf["pos"][mp[js]].astype(np.float64), obs, gc.INV_LEVEL_SIGMA2[kps["octave"][js]].astype(np.float64),
                                                      frame["K"].astype(np.float64))
        outlier[js] = outl != 0
        T2 = np.zeros(16, np.float32)
        h.ccmh_se3quat_to_cvmat(_p(np.ascontiguousarray(cam, np.float64)), _p(T2))
        T = T2
        return ninl

    def search(th, orb_dist):
        nonlocal mp
        r = gc.replay(dict(frame, mp=mp), T.reshape(4, 4), dict(kf, found=found), th, orb_dist, True)
        mp = r["mp"]
        return r["nmatches"]

    n_good = trace[0] = optimise()
    if n_good >= 10:
        mp[outlier] = -1
        if n_good < 50:
            nadd = trace[1] = search(10.0, 100)
            if nadd + n_good >= 50:
                n_good = trace[2] = optimise()
                if 30 < n_good < 50:
                    found[:] = 0
                    found[mp[mp >= 0]] = 1
                    nadd = trace[3] = search(3.0, 64)
                    if n_good + nadd >= 50:
                        n_good = trace[4] = optimise()
                        mp[outlier] = -1
    return dict(matched=n_good >= 50, n_good=n_good, Tcw=T.reshape(4, 4), mp=mp, trace=trace)


@pytest.mark.parametrize("path", gc.REFINE_PATHS)
def test_refine_chain(ctx, path):
    sc = gc.refine_scene(path)
    frame, kf = sc["frame"], sc["kf"]
    assert 140 <= len(kf["live"]) <= 160 and 380 <= len(frame["kps"]) <= 420
    want = compose_refine(ctx, sc)
    t = want["trace"]
    print(path, "trace", t, "n_good", want["n_good"])
    if path == "few":
        assert 0 <= t[0] < 10 and t[1:] == [-1] * 4 and not want["matched"]
    elif path == "first":
        assert t[0] >= 50 and t[1:] == [-1] * 4 and want["matched"]
    elif path == "widen1":
        assert 10 <= t[0] < 50 and t[0] + t[1] >= 50 and t[2] >= 50 and t[3:] == [-1, -1] and want["matched"]
    else:
        assert 10 <= t[0] < 50 and t[0] + t[1] >= 50 and 30 < t[2] < 50 and t[2] + t[3] >= 50 and t[4] >= 50 and want["matched"]
    got = reloc.refine(ctx, frame["K"], gc.W, gc.H, frame["kps"], frame["desc"], gc.INV_LEVEL_SIGMA2, pose_of(sc["T0"]), kf_of(kf), sc["matches_f"], sc["inliers"])
    assert list(got.trace) == t and got.n_good == want["n_good"] and got.matched == want["matched"]
    assert np.array_equal(got.map_points, want["mp"])
    assert gc.same_float_bits(got.Tcw, want["Tcw"])
