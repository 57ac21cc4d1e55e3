"""GPU: ccm_sim3_correct_map against the numpy checker of test_sim3_correct_cpu.py (bit-identical), both forms, the edge shapes, the host mirror on a context
against the host mirror without one, every CCM_E_ARG case and two contexts on two threads."""
import threading

import numpy as np
import pytest

from test_sim3_correct_cpu import KEYS, assert_same, bad_arguments, check_flat, same_bits

f32 = np.float32


@pytest.fixture(scope="module")
def S():
    from ccm_slam_amd import sim3_correct
    return sim3_correct


_SCENES = {}


def _scene(S, size):
    """scene, flat arguments and the checker's answer of one of the three sizes, computed once"""
    if size not in _SCENES:
        n_kf, n_pt = S.SIZES[size]
        sc = S.make_scene(seed=100 + n_kf, n_kf=n_kf, n_pt=n_pt)
        f = S.flatten_loop(sc)
        _SCENES[size] = (sc, f, check_flat(f))
    return _SCENES[size]


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["loop", "agent", "agents4"])
def test_device_matches_the_checker(ctx, S, size):
    sc, f, exp = _scene(S, size)
    n_kf, n_pt = S.SIZES[size]
    assert f["sel"].size > 0.8 * n_pt and 5 * f["sel"].size < f["obs_kf"].size < 8 * f["sel"].size
    assert_same(S.correct_map(ctx, f), exp, size)
    # epilogue form: the loop form's tables, the corrected ones moved a little further; a point moves with its reference keyframe
    rng = np.random.default_rng(7)
    S_cor = exp["S_cor"] * (1 + 1e-3 * rng.normal(size=exp["S_cor"].shape))
    g = S.flatten_epilogue(sc, exp["S_non"], S_cor, np.where(np.asarray(sc["ref_kf"]) < n_kf, sc["ref_kf"], -1))
    got = S.correct_map(ctx, g)
    assert_same(got, check_flat(g), size + " epilogue")
    assert same_bits(got["S_cor"], S_cor) and same_bits(got["S_non"], exp["S_non"])        # inputs of this form: handed back untouched


def _tiny(S, **kw):
    a = dict(seed=31, n_kf=5, n_pt=130, n_out=3, window=8, mean_obs=3.0)
    a.update(kw)
    return S.make_scene(**a)


@pytest.mark.gpu
def test_edge_shapes(ctx, S):
    # keyframes only
    f = S.flatten_loop(_tiny(S))
    g = dict(f); g["n_pt"] = 0
    out = S.correct_map(ctx, g)
    exp = check_flat(f)
    for k in ("Tiw", "center", "S_non", "S_cor"):
        assert same_bits(out[k].reshape(exp[k].shape), exp[k]), k
    g = dict(f, n_pt=0, pos=np.zeros(0, f32), owner=None, owner_rank=None, obs_off=None, obs_kf=None, ref_kf=None, ref_level=None)
    out2 = S.correct_map(ctx, g)                                                                   # ... with the per-point pointers NULL
    assert same_bits(out2["Tiw"], out["Tiw"])
    # one keyframe (the current one), observers outside it; one point
    sc = S.make_scene(seed=32, n_kf=1, n_pt=70, n_out=6, window=7, mean_obs=4.0)
    f = S.flatten_loop(sc)
    assert f["sel"].size > 10
    assert_same(S.correct_map(ctx, f), check_flat(f), "one keyframe")
    sc = _tiny(S, n_pt=1, no_obs_frac=0, bad_frac=0, tagged_frac=0, stale_frac=0, null_frac=0)
    f = S.flatten_loop(sc)
    assert f["sel"].size == 1
    assert_same(S.correct_map(ctx, f), check_flat(f), "one point")
    # more than one workgroup with a ragged tail, a point with 30 observers among points with 2, all eight octaves
    sc = S.make_scene(seed=33, n_kf=40, n_pt=64 * 3 + 5, n_out=0, window=40, mean_obs=2.0, no_obs_frac=0, stale_frac=0, bad_frac=0, tagged_frac=0)
    cnt = np.diff(sc["obs_off"])
    assert (cnt == 2).sum() > 20 and cnt.max() < 30
    big = int(np.argmax(cnt == 2))                                                                 # give one of them 30 observers
    off = np.asarray(sc["obs_off"]).copy(); okf = np.asarray(sc["obs_kf"])
    extra = np.setdiff1d(np.arange(40), okf[off[big]:off[big + 1]])[:28].astype(np.int32)
    sc["obs_kf"] = np.concatenate([okf[:off[big + 1]], extra, okf[off[big + 1]:]])
    off[big + 1:] += 28
    sc["obs_off"] = off
    f = S.flatten_loop(sc)
    assert np.diff(f["obs_off"]).max() == 30 and set(np.asarray(f["ref_level"])) == set(range(8))
    assert_same(S.correct_map(ctx, f), check_flat(f), "30 next to 2")


@pytest.mark.gpu
def test_nan_and_inf_positions_propagate(ctx, S):
    sc = _tiny(S)
    pos = np.asarray(sc["pos"], f32).reshape(-1, 3).copy()
    a, b, c, d, e = (int(x) for x in S.flatten_loop(sc)["sel"][[3, 10, 20, 30, 40]])            # points that are corrected
    pos[a, 0] = np.nan; pos[b] = np.inf; pos[c, 2] = -np.inf; pos[d] = 3e38; pos[e] = 0
    sc["pos"] = pos
    f = S.flatten_loop(sc)
    got = S.correct_map(ctx, f)
    exp = check_flat(f)
    for k in KEYS:                                                     # a NaN where the checker has one (IEEE 754 leaves its sign and payload open), the same bits elsewhere
        g = np.asarray(got[k]).reshape(exp[k].shape)
        nan = np.isnan(exp[k])
        assert np.array_equal(np.isnan(g), nan), k
        assert same_bits(np.where(nan, 0, g), np.where(nan, 0, exp[k])), k
    at = {int(p): i for i, p in enumerate(f["sel"])}
    assert np.isnan(got["pos"][at[a]]).any() and not np.isfinite(got["pos"][at[b]]).any()
    ok = np.ones(f["sel"].size, bool); ok[[at[p] for p in (a, b, c, d)]] = False
    assert np.isfinite(got["pos"][ok]).all() and np.isfinite(got["normal"][ok]).all()
    assert_same(S.correct_map(ctx, S.flatten_loop(_tiny(S))), check_flat(S.flatten_loop(_tiny(S))), "the context works afterwards")


@pytest.mark.gpu
def test_host_mirror_on_a_context_equals_the_host_mirror_without(S):
    sc = S.make_scene(seed=34, n_kf=30, n_pt=1500)
    a = S.MapCorrection.loop(sc, device=0); b = S.MapCorrection.loop(sc)
    ra, rb = a.results(), b.results()
    a.close(); b.close()
    for k in KEYS + ("tag",):
        assert same_bits(ra[k], rb[k]), k
    assert (ra["tag"] >= 0).sum() > 1000 and (ra["tag"] < 0).any()
    pt_kf = np.where(np.asarray(sc["ref_kf"]) < 30, sc["ref_kf"], ra["tag"])
    a = S.MapCorrection.epilogue(sc, ra["S_non"], ra["S_cor"] * 1.0005, pt_kf, device=0); b = S.MapCorrection.epilogue(sc, ra["S_non"], ra["S_cor"] * 1.0005, pt_kf)
    ra, rb = a.results(), b.results()
    a.close(); b.close()
    for k in KEYS + ("tag",):
        assert same_bits(ra[k], rb[k]), k


@pytest.mark.gpu
def test_error_paths(ctx, S):
    from ccm_slam_amd._lib import CcmError, lib
    sc = S.make_scene(seed=4, n_kf=6, n_pt=50, n_out=2, window=8)
    good = S.flatten_loop(sc)
    exp = check_flat(good)
    assert_same(S.correct_map(ctx, good), exp)
    for key, val in bad_arguments(good):
        f = dict(good); f[key] = val
        with pytest.raises(CcmError):
            S.correct_map(ctx, f)
    # each pointer in turn as NULL, through the raw entry
    import ctypes as C
    keep = {k: np.ascontiguousarray(np.asarray(good[k], dt).reshape(-1)) for k, dt in
            (("Tiw", f32), ("Twc", f32), ("Scw", np.float64), ("kf_center", f32), ("kf_rank", np.int32), ("pos", f32), ("owner", np.int32), ("owner_rank", np.int32),
             ("obs_off", np.int32), ("obs_kf", np.int32), ("ref_kf", np.int32), ("ref_level", np.int32), ("scale_factors", f32), ("normal", f32), ("min_dist", f32),
             ("max_dist", f32))}
    n_pt = keep["pos"].size // 3
    outs = dict(S_non=np.zeros(48), S_cor=np.zeros(48), pos_out=np.zeros(3 * n_pt, f32), Tiw_new=np.zeros(72, f32), center_new=np.zeros(18, f32))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    full = [6, p(keep["Tiw"]), int(good["cur"]), p(keep["Twc"]), p(keep["Scw"]), p(outs["S_non"]), p(outs["S_cor"]), 8, p(keep["kf_center"]), p(keep["kf_rank"]), n_pt,
            p(keep["pos"]), p(keep["owner"]), p(keep["owner_rank"]), p(keep["obs_off"]), p(keep["obs_kf"]), p(keep["ref_kf"]), p(keep["ref_level"]),
            p(keep["scale_factors"]), 8, p(outs["pos_out"]), p(keep["normal"]), p(keep["min_dist"]), p(keep["max_dist"]), p(outs["Tiw_new"]), p(outs["center_new"])]
    fn = lib().ccm_sim3_correct_map
    assert fn(ctx.handle, *full) == 0 and same_bits(outs["pos_out"].reshape(-1, 3), exp["pos"])
    for i in (3, 4, 5, 6, 8, 9, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 22, 23, 24, 25):
        a = list(full); a[i] = None
        assert fn(ctx.handle, *a) == -1, i
    assert fn(None, *full) == -1
    # the epilogue form needs no current keyframe
    g = S.flatten_epilogue(sc, exp["S_non"], exp["S_cor"], np.where(np.asarray(sc["ref_kf"]) < 6, sc["ref_kf"], -1))
    g["cur"] = -5
    assert_same(S.correct_map(ctx, g), check_flat(g))
    assert_same(S.correct_map(ctx, good), exp, "the context works after the errors")


@pytest.mark.gpu
def test_two_threads_with_their_own_contexts(S):
    from ccm_slam_amd._lib import Context
    flats = [S.flatten_loop(S.make_scene(seed=60 + i, n_kf=40 + 10 * i, n_pt=2500 + 700 * i)) for i in range(2)]
    want = [check_flat(f) for f in flats]
    out = [None, None]
    err = []

    def worker(i):
        try:
            c = Context(0)
            out[i] = [S.correct_map(c, flats[i]) for _ in range(5)]
            c.close()
        except Exception as e:   # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for i in range(2):
        for r in out[i]:
            assert_same(r, want[i], f"thread {i}")
