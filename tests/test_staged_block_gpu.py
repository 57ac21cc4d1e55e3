"""GPU: the five staged stages interleaved on ONE context, at sizes that grow and then shrink, so that the device scratch and the pinned block are
regrown between stages and then reused at a smaller size; a triangulation and a Sim3 correction start right behind a ccm_frame_set_keypoints and a
ccm_pose_optimize call, i.e. on a stream that is still busy.  Every result equals what the same call gives on a fresh context and what the host evaluator or
checker of the stage's own test file gives (exact, as there)."""
import numpy as np
import pytest

from test_culling_cpu import assert_same as kfcull_same
from test_covis_cpu import assert_same as covis_same
from test_sim3_correct_cpu import assert_same as s3c_same, check_flat
from test_sim3_ransac_gpu import _cands, _compare_rts, _random_hyps, ref_hypothesis
from test_triangulate_cpu import ref_pairs, same_bits


def _fresh(call):
    from ccm_slam_amd._lib import Context
    c = Context(0)
    try:
        return call(c)
    finally:
        c.close()


def _covis(ctx, n_kf):
    from ccm_slam_amd import covis as V
    sc = V.make_scene(seed=40 + n_kf, n_kf=n_kf, n_out=3, n_pt=20 * n_kf + 40, window=min(n_kf + 3, 40))
    got = V.update(ctx, sc)
    covis_same(got, _fresh(lambda c: V.update(c, sc)), f"covis {n_kf}: against a fresh context")
    covis_same(got, V.update_host(sc), f"covis {n_kf}: against the host evaluator")
    return got


def _kfcull(ctx, seed, n_cand, n_pt, **kw):
    from ccm_slam_amd import culling as K
    sc = K.make_scene(seed=seed, n_cand=n_cand, n_pt=n_pt, **kw)
    got = K.walk(ctx, sc, thres=0.9)
    for name, want in (("a fresh context", _fresh(lambda c: K.walk(c, sc, thres=0.9))), ("the host evaluator", K.walk_host(sc, thres=0.9))):
        kfcull_same(got, want, f"kfcull {n_cand}: against {name}")
        assert got["n_reeval"] == want["n_reeval"], (n_cand, name)
    return sc, got


def _sim3_correct(ctx, f, tag):
    from ccm_slam_amd import sim3_correct as S
    got = S.correct_map(ctx, f)
    s3c_same(got, _fresh(lambda c: S.correct_map(c, f)), f"sim3_correct {tag}: against a fresh context")
    return got


def _triangulate(ctx, sc, tag):
    from ccm_slam_amd import triangulate as T
    args = T.flat(sc)
    st, x3d, nacc = T.triangulate_pairs(ctx, *args)
    fst, fx3d, fnacc = _fresh(lambda c: T.triangulate_pairs(c, *args))
    assert np.array_equal(st, fst) and same_bits(x3d, fx3d) and list(nacc) == list(fnacc), f"triangulate {tag}: against a fresh context"
    rst, rx = ref_pairs(*args)
    assert np.array_equal(st, rst) and same_bits(x3d, rx), f"triangulate {tag}: against the checker"
    off = np.asarray(args[2])
    assert list(nacc) == [int((rst[off[s]:off[s + 1]] == 0).sum()) for s in range(off.size - 1)], tag
    return st


def _sim3_ransac(ctx, cands, hc, hi, tag):
    from ccm_slam_amd import sim3
    n, rts, masks = sim3.eval_hypotheses(ctx, cands, hc, hi)
    fn, frts, fmasks = _fresh(lambda c: sim3.eval_hypotheses(c, cands, hc, hi))
    assert np.array_equal(n, fn) and same_bits(rts, frts) and all(np.array_equal(a, b) for a, b in zip(masks, fmasks)), f"sim3_ransac {tag}: against a fresh context"
    for h in range(len(hc)):
        ni, ref, inl = ref_hypothesis(cands[hc[h]], hi[h], False)
        assert n[h] == ni and np.array_equal(masks[h], inl), (tag, h)
        _compare_rts(rts[h], ref)
    return n


def _busy(ctx, fg, kps, desc, pose):
    """leaves the context's stream with work in flight: the keypoint upload and grid build of a frame, then a pose optimisation"""
    from ccm_slam_amd import optimizer
    fg.set_keypoints(kps, desc)
    optimizer.pose_optimization(ctx, pose["cam_qt"], pose["Xw"], pose["obs"], pose["info"], pose["K"])


@pytest.mark.gpu
def test_five_stages_interleaved_on_one_context_growing_then_shrinking():
    from ccm_slam_amd import sim3_correct as S, synth, triangulate as T
    from ccm_slam_amd._lib import Context
    from ccm_slam_amd.frame import FrameGrid
    rng = np.random.default_rng(9)
    kps = np.zeros(1500, dtype=[("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
    kps["x"] = rng.uniform(20, 730, kps.size); kps["y"] = rng.uniform(20, 460, kps.size); kps["octave"] = rng.integers(0, 8, kps.size)
    desc = rng.integers(0, 256, (kps.size, 32), dtype=np.uint8)
    pose = synth.make_pose_problem(n=300, seed=3)
    # the Sim3 correction at its loop size and without points, and its checker's answers (computed once)
    n_kf, n_pt = S.SIZES["loop"]
    f_loop = S.flatten_loop(S.make_scene(seed=100 + n_kf, n_kf=n_kf, n_pt=n_pt))
    exp_loop = check_flat(f_loop)
    f_tiny = S.flatten_loop(S.make_scene(seed=31, n_kf=5, n_pt=130, n_out=3, window=8, mean_obs=3.0))
    exp_tiny = check_flat(f_tiny)
    f_none = dict(f_tiny, n_pt=0)
    # Sim3 RANSAC: one hypothesis, and a few hundred over candidates of 20 .. 1000 points
    cands = _cands(77, 1, 2, [20, 65, 1000])
    hc1, hi1 = _random_hyps(np.random.default_rng(1), cands[:1], 1)
    hcN, hiN = _random_hyps(np.random.default_rng(2), cands, 300)
    tri_one = T.make_pair_scene(seed=230, S=1, n_pairs=1, mismatch=0, behind=0, tiny_baseline=0, wild_octave=0)
    tri_many = T.make_pair_scene(seed=233, S=9, n_pairs=333)
    assert tri_many["pair_off"][-1] == 2997

    ctx = Context(0)
    fg = FrameGrid(ctx, synth.EUROC_K, np.zeros(4, np.float32), 752, 480)
    try:
        def small(tag):
            _covis(ctx, 2)
            _, got = _kfcull(ctx, 21, 1, 60, n_out=5, window=6, skip_frac=0, not_erase_frac=0)
            assert got["n_mps"][0] > 0
            _sim3_ransac(ctx, cands[:1], hc1, hi1, tag)
            assert _triangulate(ctx, tri_one, tag).size == 1
            none = _sim3_correct(ctx, f_none, tag)
            for k in ("Tiw", "center", "S_non", "S_cor"):
                assert same_bits(none[k].reshape(exp_tiny[k].shape), exp_tiny[k]), (tag, k)

        small("first, on an empty scratch")
        # growing: every stage now needs more scratch and a larger pinned block than the one before it left
        assert _covis(ctx, 70)["col"].size > 70
        sc, got = _kfcull(ctx, 31, 40, 5400, n_out=14, window=16)
        assert np.diff(sc["list_off"]).min() > 256 and (got["verdict"] == 1).any()
        _busy(ctx, fg, kps, desc, pose)
        s3c_same(_sim3_correct(ctx, f_loop, "loop, behind a busy stream"), exp_loop, "sim3_correct loop: against the checker")
        assert _sim3_ransac(ctx, cands, hcN, hiN, "300 hypotheses").max() > 3
        _busy(ctx, fg, kps, desc, pose)
        assert (_triangulate(ctx, tri_many, "2997 pairs, behind a busy stream") == 0).sum() > 1000
        # shrinking: the same small calls in the buffers the large ones left behind
        small("again, in the grown buffers")
    finally:
        fg.close()
        ctx.close()
