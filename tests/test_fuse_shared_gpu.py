"""GPU: the two batched Fuse stages agree where they must.  On the scene of tests/fuse_shared_cases.py (3 keyframes x 300 points: a full tile,
a tail of 44, a partly dead last wave; windows on both sides of the wave switch) ccm_fuse_pose_eval equals ccm_fuse_sim3_eval bit for bit, and both equal the host
evaluator: table, n_valid, n_hit and uv.  fuse_sim3_kernel and fuse_pose_kernel are two wrappers around one pair body (csrc/fuse.hip); this holds them to it."""
import pytest

from ccm_slam_amd import fuse_pose as fp, fuse_sim3 as fs
from fuse_shared_cases import assert_not_vacuous, pose_scene, same_bits, sim3_scene

pytestmark = pytest.mark.gpu


def test_pose_stage_equals_sim3_stage_and_the_host_evaluator_on_the_shared_scene(ctx):
    sc = sim3_scene()
    ps = pose_scene(sc)
    want = fs.fuse_sim3_eval_host(sc, want_uv=True, want_cand=True)
    assert_not_vacuous(want)
    dev_sim3 = fs.fuse_sim3_eval(ctx, sc, want_uv=True)
    dev_pose = fp.fuse_pose_eval(ctx, ps, want_uv=True)
    same_bits(dev_sim3, dev_pose, "device pose against device sim3")
    same_bits(want, dev_pose, "device pose against host sim3")
    same_bits(dev_sim3, fp.fuse_pose_eval_host(ps, want_uv=True), "host pose against device sim3")
