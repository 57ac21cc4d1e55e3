"""GPU: ccm_fuse_pose_eval as a staged stage among the others on ONE context: interleaved with ccm_fuse_sim3_eval, ccm_triangulate_pairs and
ccm_covis_update at sizes that grow and then shrink, so that the device scratch and the pinned block are regrown and then reused at a smaller size, and right
behind a ccm_frame_set_keypoints call, i.e. on a stream that still has the pinned block in flight.  Every result equals the host evaluator's (exact)."""
import numpy as np
import pytest

from test_fuse_pose_gpu import same
from test_fuse_sim3_gpu import same as same_sim3
from test_staged_block_gpu import _covis, _triangulate


@pytest.mark.gpu
def test_fuse_pose_calls_interleaved_with_other_staged_stages():
    from ccm_slam_amd import fuse_pose as fp, fuse_sim3 as fs, synth, triangulate as T
    from ccm_slam_amd._lib import Context
    from ccm_slam_amd.frame import FrameGrid
    rng = np.random.default_rng(9)
    kps = np.zeros(1500, dtype=[("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
    kps["x"] = rng.uniform(20, 730, kps.size); kps["y"] = rng.uniform(20, 460, kps.size); kps["octave"] = rng.integers(0, 8, kps.size)
    desc = rng.integers(0, 256, (kps.size, 32), dtype=np.uint8)
    jobs = {}
    for tag, (calls, p1, p2, F, uv) in dict(tiny=(1, 1, 1, 30, True), mid=(3, 257, 300, 400, False), big=(25, 1000, 8000, 1000, True)).items():
        sc = fp.make_scene(calls, p1, p2, n_feat=F, seed=60 + calls)
        jobs[tag] = (sc, uv, fp.fuse_pose_eval_host(sc, want_uv=uv))
    assert jobs["big"][2]["n_hit"].min() > 100 and jobs["big"][2]["n_hit"][-1] > 3000
    sim3 = fs.make_scene(6, 700, n_feat=500, seed=5)
    sim3_want = fs.fuse_sim3_eval_host(sim3, want_uv=True)
    tri_one = T.make_pair_scene(seed=230, S=1, n_pairs=1, mismatch=0, behind=0, tiny_baseline=0, wild_octave=0)
    tri_many = T.make_pair_scene(seed=233, S=9, n_pairs=333)

    ctx = Context(0)
    fg = FrameGrid(ctx, synth.EUROC_K, np.zeros(4, np.float32), 752, 480)
    try:
        def fuse(tag, note):
            sc, uv, want = jobs[tag]
            same(fp.fuse_pose_eval(ctx, sc, want_uv=uv), want, f"fuse {tag}: {note}")

        def fuse_sim3(note):
            same_sim3(fs.fuse_sim3_eval(ctx, sim3, want_uv=True), sim3_want, f"fuse_sim3: {note}")

        fuse("tiny", "first, on an empty scratch")
        _triangulate(ctx, tri_one, "one pair"); _covis(ctx, 2); fuse_sim3("after the tiny call")
        # growing
        fuse("mid", "growing")
        _covis(ctx, 70)
        fuse("big", "growing further")
        _triangulate(ctx, tri_many, "2997 pairs")
        fg.set_keypoints(kps, desc)
        fuse("big", "right behind a keypoint upload")
        fuse_sim3("in the grown buffers")
        # shrinking: small calls in the buffers the large ones left behind
        fuse("tiny", "in the grown buffers"); fuse("mid", "in the grown buffers")
        _covis(ctx, 2)
        fg.set_keypoints(kps, desc)
        fuse("mid", "shrunk, behind a keypoint upload"); fuse("tiny", "shrunk")
        _triangulate(ctx, tri_one, "one pair again"); fuse_sim3("between two pose calls")
        fuse("big", "grown again")
    finally:
        fg.close()
        ctx.close()
