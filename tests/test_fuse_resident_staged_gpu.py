"""GPU: the resident Fuse calls as staged stages among the others on ONE context: interleaved with ccm_triangulate_pairs, ccm_covis_update
and the stateless ccm_fuse_sim3_eval / ccm_fuse_pose_eval, and with adds to and erases from the store, at sizes that grow and then shrink, so that the device scratch and the pinned block are
regrown and then reused at a smaller size, and right behind a ccm_frame_set_keypoints call, i.e. on a stream that still has the pinned block in flight.  Every
result equals the host evaluator's (exact)."""
import numpy as np
import pytest

from kfstore_cases import same_result
from test_staged_block_gpu import _covis, _triangulate


@pytest.mark.gpu
def test_resident_fuse_calls_interleaved_with_other_staged_stages():
    from ccm_slam_amd import fuse_pose as fp, fuse_sim3 as fs, kfstore as ks, synth, triangulate as T
    from ccm_slam_amd._lib import Context
    from ccm_slam_amd.frame import FrameGrid
    rng = np.random.default_rng(9)
    kps = np.zeros(1500, dtype=[("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
    kps["x"] = rng.uniform(20, 730, kps.size); kps["y"] = rng.uniform(20, 460, kps.size); kps["octave"] = rng.integers(0, 8, kps.size)
    desc = rng.integers(0, 256, (kps.size, 32), dtype=np.uint8)
    jobs = {}
    for tag, (K, P, F, uv) in dict(tiny=(1, 1, 30, True), mid=(3, 257, 400, False), big=(40, 2000, 1000, True)).items():
        sc = fs.make_scene(K, P, n_feat=F, seed=60 + K)
        jobs[tag] = (sc, uv, fs.fuse_sim3_eval_host(sc, want_uv=uv))
    assert jobs["big"][2]["n_hit"].max() > 500
    pose = fp.make_scene(6, 300, 900, n_feat=500, seed=5)
    pose_want = fp.fuse_pose_eval_host(pose, want_uv=True)
    tri_one = T.make_pair_scene(seed=230, S=1, n_pairs=1, mismatch=0, behind=0, tiny_baseline=0, wild_octave=0)
    tri_many = T.make_pair_scene(seed=233, S=9, n_pairs=333)

    ctx = Context(0)
    fg = FrameGrid(ctx, synth.EUROC_K, np.zeros(4, np.float32), 752, 480)
    store = ks.KeyFrameStore(ctx, 64, 1000)
    base = dict(tiny=0, mid=10, big=20)
    try:
        for tag, (sc, _, _) in jobs.items():
            store.add_scene(range(base[tag], base[tag] + sc.K), sc)

        def resident(tag, note):
            sc, uv, want = jobs[tag]
            same_result(ks.fuse_sim3_eval_resident(ctx, store, range(base[tag], base[tag] + sc.K), sc, want_uv=uv), want, f"resident {tag}: {note}")

        def stateless(tag, note):
            sc, uv, want = jobs[tag]
            same_result(fs.fuse_sim3_eval(ctx, sc, want_uv=uv), want, f"stateless {tag}: {note}")

        def resident_pose(note):
            same_result(ks.fuse_pose_eval_resident(ctx, store, range(70, 70 + pose.K), pose, want_uv=True), pose_want, f"resident pose: {note}")

        resident("tiny", "first, on an empty scratch")
        _triangulate(ctx, tri_one, "one pair"); _covis(ctx, 2)
        # growing
        resident("mid", "growing")
        _covis(ctx, 70)
        resident("big", "growing further")
        stateless("big", "the stateless call behind the resident one")
        _triangulate(ctx, tri_many, "2997 pairs")
        fg.set_keypoints(kps, desc)
        resident("big", "right behind a keypoint upload")
        store.erase(base["tiny"])
        store.add_scene(range(70, 70 + pose.K), pose)          # an add between the calls: it reuses the erased slot
        store.add_scene([base["tiny"]], jobs["tiny"][0])
        resident_pose("after an add")
        same_result(fp.fuse_pose_eval(ctx, pose, want_uv=True), pose_want, "stateless pose")
        # shrinking: small calls in the buffers the large ones left behind
        resident("tiny", "in the grown buffers"); resident("mid", "in the grown buffers")
        _covis(ctx, 2)
        fg.set_keypoints(kps, desc)
        resident("mid", "shrunk, behind a keypoint upload"); resident("tiny", "shrunk")
        stateless("tiny", "shrunk")
        _triangulate(ctx, tri_one, "one pair again")
        resident_pose("shrunk")
        resident("big", "grown again")
    finally:
        store.close()
        fg.close()
        ctx.close()
