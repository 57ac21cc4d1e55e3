"""The two batched Fuse stages agree where they must, on the CPU: on the scene of tests/fuse_shared_cases.py (the Sim3 scene with pose = the
decomposed Scw, inv_level_sigma2 = 0 and the jobs (k, 0, P)) fuse_pose_eval_host equals fuse_sim3_eval_host bit for bit: table, n_valid, n_hit, uv and n_cand.
Both run one pair body, one candidate and one window walk (csrc/fuse_math.h, host/ccm_host.cpp); this holds them to it."""
from ccm_slam_amd import fuse_pose as fp, fuse_sim3 as fs
from fuse_shared_cases import assert_not_vacuous, pose_scene, same_bits, sim3_scene


def test_pose_host_evaluator_equals_sim3_host_evaluator_on_the_shared_scene():
    sc = sim3_scene()
    want = fs.fuse_sim3_eval_host(sc, want_uv=True, want_cand=True)
    assert_not_vacuous(want)
    same_bits(want, fp.fuse_pose_eval_host(pose_scene(sc), want_uv=True, want_cand=True), "host", cand=True)
