"""The guided search of relocalisation on the CPU: the host evaluator of ccm_frame_guided_search (csrc/guided_search_math.h with a host grid) and the mirror's sequential
pass against tests/guided_search_cases.py's line-by-line replay of ORBmatcher.cpp:1478-1604.  Every comparison is equality of integers or of float bits."""
import os
import subprocess

import numpy as np
import pytest

import guided_search_cases as gc
from ccm_slam_amd import reloc
from guided_search_cases import assert_evaluation, host_eval, host_mirror, kf_of, pose_of, skip_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def scenes():
    out = []
    for seed in SEEDS:
        frame, T, kf = gc.random_scene(seed)
        out.append((frame, T, kf, {th: gc.replay(frame, T, kf, th, 100 if th == 10.0 else 64, True) for th in (10.0, 3.0)}))
    return out


def test_the_scenes_exercise_the_search(scenes):
    """asserted on the replay alone: every status, a point behind the camera inside the image, 30 matches, a match the rotation check takes back"""
    for frame, T, kf, rs in scenes:
        r = rs[10.0]
        assert set(r["status"]) == {gc.SKIPPED, gc.OUTSIDE, gc.RANGE, gc.SEARCHED}
        assert np.any((r["zc"] < 0) & (r["status"] == gc.SEARCHED))
        assert r["nmatches"] >= 30 and r["removed"] >= 1
        assert np.any(r["level"] == 0) and np.any(r["level"] == gc.N_LEVELS - 1)


def test_host_evaluator_equals_the_replay(scenes):
    for frame, T, kf, rs in scenes:
        for th, r in rs.items():
            assert_evaluation(host_eval(frame, T, kf, th), r, th)


@pytest.mark.parametrize("ori", [True, False])
def test_host_mirror_equals_the_replay(scenes, ori):
    for frame, T, kf, rs in scenes:
        for th, orb_dist in ((10.0, 100), (3.0, 64)):
            r = rs[th] if ori else gc.replay(frame, T, kf, th, orb_dist, False)
            n, mp = host_mirror(frame, T, kf, th, orb_dist, ori)
            assert n == r["nmatches"] and np.array_equal(mp, r["mp"])


@pytest.mark.parametrize("case", gc.edge_cases(), ids=lambda c: c[0])
def test_planted_edge(case):
    name, frame, T, kf, th, orb_dist, ori, expect = case
    r = gc.replay(frame, T, kf, th, orb_dist, ori)
    expect(r)
    assert_evaluation(host_eval(frame, T, kf, th), r, name)
    n, mp = host_mirror(frame, T, kf, th, orb_dist, ori)
    assert n == r["nmatches"] and np.array_equal(mp, r["mp"])


def test_sizing_call_and_short_capacity(scenes):
    frame, T, kf, rs = scenes[0]
    r = rs[10.0]
    total = int(r["idx"].size)
    args = (frame["kps"], frame["desc"], frame["bounds"], frame["K"], pose_of(T), kf["pos"], kf["dmin"], kf["dmax"], kf["desc"], skip_of(kf), 10.0)
    got = reloc.guided_search_host(*args, cap=0)
    assert got["n_cand"] == total and np.array_equal(got["off"], r["off"]) and got["idx"].size == 0
    assert_evaluation(reloc.guided_search_host(*args, cap=total), r, "exact capacity")
    with pytest.raises(reloc.CcmError) as e:
        reloc.guided_search_host(*args, cap=total - 1)
    assert e.value.n_cand == total


def test_bad_arguments_of_the_host_forms(scenes):
    frame, T, kf, _ = scenes[0]
    base = (frame["kps"], frame["desc"], frame["bounds"], frame["K"])
    pts = (kf["pos"], kf["dmin"], kf["dmax"], kf["desc"], skip_of(kf))
    for n_levels in (0, 17, -1):
        with pytest.raises(reloc.CcmError):
            reloc.guided_search_host(*base, reloc.guided_pose(T, gc.LOG_SF, gc.SF, n_levels), *pts, 10.0)
    for th in (-1.0, float("nan"), float("inf")):
        with pytest.raises(reloc.CcmError):
            reloc.guided_search_host(*base, pose_of(T), *pts, th)
    for orb_dist in (-1, 256):
        with pytest.raises(reloc.CcmError):
            reloc.search_by_projection_kf_host(*base, pose_of(T), kf_of(kf), kf["found"], 10.0, orb_dist, True, frame["mp"])


def test_projection_equals_the_compiled_reference(scenes, oracle_lib):
    """Frame::isInFrustum of the compiled reference restatement computes the same two expressions: for the points it accepts with cos_limit = -2, its proj_x / proj_y
    are the new u / v bit for bit (a double quotient rounded to float is the float quotient).  dist3D and the level are not compared: the two camera centres differ."""
    n = 0
    for frame, T, kf, rs in scenes:
        r = rs[10.0]
        T34 = np.asarray(T, np.float32)[:3]
        frame24 = np.concatenate([T34[:, :3].reshape(-1), T34[:, 3], gc.camera_centre(T34), frame["K"],
                                  [frame["bounds"][0], frame["bounds"][2], frame["bounds"][1], frame["bounds"][3]], [gc.LOG_SF]]).astype(np.float32)
        inv, px, py, _, _ = oracle_lib.is_in_frustum(frame24, gc.N_LEVELS, kf["pos"], np.tile(np.float32([0, 0, 1]), (len(kf["live"]), 1)), kf["dmin"], kf["dmax"], -2.0)
        sel = (inv != 0) & (r["status"] >= gc.OUTSIDE)
        n += int(sel.sum())
        assert gc.same_float_bits(px[sel], r["u"][sel]) and gc.same_float_bits(py[sel], r["v"][sel])
    assert n >= 100


def test_block_header_and_replay_under_the_sanitizers(tmp_path):
    """tests/host/guided_search_check.cpp: GuidedSearchBlock's layout, guided_search_math.h and the sequential pass as a stand-alone program built with the address
    and undefined-behaviour sanitizers and run as a child process"""
    exe = tmp_path / "guided_search_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe), os.path.join(HERE, "host", "guided_search_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("guided search ok") and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
