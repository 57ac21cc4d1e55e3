"""GPU: ccm_gba_apply_map as a staged stage among the others on ONE context: interleaved with ccm_sim3_correct_map and ccm_kfcull_walk at sizes
that grow and then shrink, so that the device scratch and the pinned block are regrown and then reused at a smaller size, and once right behind a
ccm_frame_set_keypoints call, i.e. on a stream that still has the pinned block in flight.  Every result equals the checker's (exact)."""
import numpy as np
import pytest

from test_culling_cpu import assert_same as kfcull_same
from test_gba_apply_cpu import assert_same, check_flat
from test_sim3_correct_cpu import assert_same as s3c_same, check_flat as s3c_check


@pytest.mark.gpu
def test_gba_apply_interleaved_with_other_staged_stages():
    from ccm_slam_amd import culling as K, gba_apply as G, sim3_correct as S, synth
    from ccm_slam_amd._lib import Context
    from ccm_slam_amd.frame import FrameGrid
    rng = np.random.default_rng(9)
    kps = np.zeros(1500, dtype=[("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
    kps["x"] = rng.uniform(20, 730, kps.size); kps["y"] = rng.uniform(20, 460, kps.size); kps["octave"] = rng.integers(0, 8, kps.size)
    desc = rng.integers(0, 256, (kps.size, 32), dtype=np.uint8)
    gba = {}
    for tag, (n_kf, n_pt, kw) in dict(tiny=(30, 70, {}), mid=(120, 4000, {}), big=(500, 37500, {}), wide=(360, 500, dict(wide_level=300, extra_nonvert=0))).items():
        f = G.flatten(G.make_scene(seed=300 + n_kf, n_kf=n_kf, n_pt=n_pt, **kw))
        gba[tag] = (f, check_flat(f))
    f_loop = S.flatten_loop(S.make_scene(seed=130, n_kf=30, n_pt=3000)); exp_loop = s3c_check(f_loop)
    f_tiny = S.flatten_loop(S.make_scene(seed=31, n_kf=5, n_pt=130, n_out=3, window=8, mean_obs=3.0)); exp_tiny = s3c_check(f_tiny)
    cull_small = K.make_scene(seed=21, n_cand=1, n_pt=60, n_out=5, window=6, skip_frac=0, not_erase_frac=0)
    cull_big = K.make_scene(seed=31, n_cand=40, n_pt=5400, n_out=14, window=16)
    cull_exp = {id(sc): K.walk_host(sc, thres=0.9) for sc in (cull_small, cull_big)}

    ctx = Context(0)
    fg = FrameGrid(ctx, synth.EUROC_K, np.zeros(4, np.float32), 752, 480)
    try:
        def apply(tag, note):
            assert_same(G.apply_map(ctx, gba[tag][0]), gba[tag][1], f"gba_apply {tag}: {note}")

        def cull(sc, note):
            kfcull_same(K.walk(ctx, sc, thres=0.9), cull_exp[id(sc)], "kfcull: " + note)

        apply("tiny", "first, on an empty scratch")
        s3c_same(S.correct_map(ctx, f_tiny), exp_tiny, "sim3_correct tiny")
        cull(cull_small, "small")
        # growing
        apply("mid", "growing")
        s3c_same(S.correct_map(ctx, f_loop), exp_loop, "sim3_correct loop")
        apply("big", "growing further")
        cull(cull_big, "big")
        fg.set_keypoints(kps, desc)
        apply("wide", "right behind a keypoint upload")
        # shrinking: small calls in the buffers the large ones left behind
        s3c_same(S.correct_map(ctx, f_tiny), exp_tiny, "sim3_correct tiny, in the grown buffers")
        apply("tiny", "again, in the grown buffers")
        cull(cull_small, "small again")
        fg.set_keypoints(kps, desc)
        apply("mid", "shrunk, behind a keypoint upload")
    finally:
        fg.close()
        ctx.close()
