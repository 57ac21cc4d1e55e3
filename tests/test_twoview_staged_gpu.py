"""GPU: ccm_twoview_ransac_eval and ccm_twoview_check_rt as staged stages among the others on ONE context: interleaved with
ccm_triangulate_pairs and ccm_sim3_ransac_eval at sizes that grow and then shrink, so that the device scratch and the pinned block are regrown and then reused
at a smaller size, and right behind a ccm_frame_set_keypoints call, i.e. on a stream that still has the pinned block in flight.  Every result equals the host
evaluator's (exact)."""
import numpy as np
import pytest

from test_sim3_ransac_gpu import _cands, _random_hyps
from test_staged_block_gpu import _sim3_ransac, _triangulate
from test_twoview_gpu import same_ransac, same_rt


@pytest.mark.gpu
def test_twoview_calls_interleaved_with_other_staged_stages():
    from ccm_slam_amd import synth, triangulate as T, twoview as tv
    from ccm_slam_amd._lib import Context
    from ccm_slam_amd.frame import FrameGrid
    rng = np.random.default_rng(9)
    kps = np.zeros(1500, dtype=[("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
    kps["x"] = rng.uniform(20, 730, kps.size); kps["y"] = rng.uniform(20, 460, kps.size); kps["octave"] = rng.integers(0, 8, kps.size)
    desc = rng.integers(0, 256, (kps.size, 32), dtype=np.uint8)
    jobs = {}
    for tag, (N, H, Q) in dict(tiny=(8, 1, 1), mid=(65, 64, 4), big=(1000, 200, 8)).items():
        sc = tv.make_scene("general", N, seed=80 + N, unmatched=N // 4, outliers=0.1 if N > 8 else 0.0)
        a = tv.ransac_inputs(sc)
        sets = tv.random_sets(N, H, N)
        Rs, ts = tv.motion_hypotheses(sc, Q)
        rec = np.stack([tv.prepare_rt(sc["K"], Rs[q], ts[q]) for q in range(Q)])
        inl = np.random.default_rng(N).random(N) < 0.9
        jobs[tag] = (sc, a, sets, rec, inl, tv.ransac_eval_host(*a, 1.0, sets), tv.check_rt_host(rec, sc["K"], sc["xy1"], sc["xy2"], inl, 4.0))
    cands = _cands(77, 1, 2, [20, 65, 1000])
    hc1, hi1 = _random_hyps(np.random.default_rng(1), cands[:1], 1)
    hcN, hiN = _random_hyps(np.random.default_rng(2), cands, 300)
    tri_one = T.make_pair_scene(seed=230, S=1, n_pairs=1, mismatch=0, behind=0, tiny_baseline=0, wild_octave=0)
    tri_many = T.make_pair_scene(seed=233, S=9, n_pairs=333)

    ctx = Context(0)
    fg = FrameGrid(ctx, synth.EUROC_K, np.zeros(4, np.float32), 752, 480)
    try:
        def ransac(tag, note):
            sc, a, sets, rec, inl, want, _ = jobs[tag]
            same_ransac(tv.ransac_eval(ctx, *a, 1.0, sets), want, f"ransac {tag}: {note}")

        def check_rt(tag, note):
            sc, a, sets, rec, inl, _, want = jobs[tag]
            same_rt(tv.check_rt(ctx, rec, sc["K"], sc["xy1"], sc["xy2"], inl, 4.0), want, f"check_rt {tag}: {note}")

        ransac("tiny", "first, on an empty scratch"); check_rt("tiny", "first")
        _sim3_ransac(ctx, cands[:1], hc1, hi1, "one hypothesis")
        _triangulate(ctx, tri_one, "one pair")
        # growing
        ransac("mid", "growing"); check_rt("mid", "growing")
        _sim3_ransac(ctx, cands, hcN, hiN, "300 hypotheses")
        ransac("big", "growing further")
        _triangulate(ctx, tri_many, "2997 pairs")
        fg.set_keypoints(kps, desc)
        check_rt("big", "right behind a keypoint upload")
        # shrinking: small calls in the buffers the large ones left behind
        check_rt("tiny", "in the grown buffers"); ransac("tiny", "in the grown buffers")
        _sim3_ransac(ctx, cands[:1], hc1, hi1, "one hypothesis again")
        fg.set_keypoints(kps, desc)
        ransac("mid", "shrunk, behind a keypoint upload"); check_rt("mid", "shrunk")
        _triangulate(ctx, tri_one, "one pair again")
    finally:
        fg.close()
        ctx.close()
