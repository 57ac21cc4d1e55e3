"""GPU: ccm_kfcull_walk against the host evaluator of the same header and against the sequential replay of test_culling_cpu.py, array for array (exact equality),
at the smallest shapes where each path can break: one and two candidates, lists longer than the workgroups of either kernel, more candidates than one word of the
erased bitmask holds, points with more observers than a lane takes alone, walks with many re-evaluations and with none, repeated calls, two contexts on two
threads, every CCM_E_ARG case and the mirror."""
import threading

import numpy as np
import pytest

from test_culling_cpu import CULLED, REDUNDANT_NOT_ERASED, assert_same, bad_calls, chain_scene, random_scene, replay_arrays


@pytest.fixture(scope="module")
def K():
    from ccm_slam_amd import culling
    return culling


def _check(ctx, K, sc, tag, thres):
    """device == host evaluator == replay, n_reeval included where both report it; returns the device's outputs"""
    got = K.walk(ctx, sc, thres=thres)
    host = K.walk_host(sc, thres=thres)
    assert_same(got, host, f"{tag}: device against the host evaluator")
    assert got["n_reeval"] == host["n_reeval"], tag
    assert_same(got, replay_arrays(sc, thres, tag=tag), f"{tag}: device against the replay")
    return got


@pytest.mark.gpu
def test_one_candidate(ctx, K):
    got = _check(ctx, K, K.make_scene(seed=21, n_cand=1, n_out=5, n_pt=60, window=6, skip_frac=0, not_erase_frac=0), "one with observers", 0.5)
    assert got["n_mps"][0] > 0 and got["n_red"][0] > 0 and got["n_reeval"] == 0
    got = _check(ctx, K, K.make_scene(seed=22, n_cand=1, n_out=0, n_pt=40, skip_frac=0, not_erase_frac=0), "one alone", 0.5)
    assert got["n_mps"][0] > 0 and got["n_red"][0] == 0 and got["verdict"].tolist() == [0]
    no_points = dict(n_cand=1, n_all=1, n_pt=0, cand_flags=np.zeros(1, np.uint8), list_off=np.array([0, 2], np.int32), list_pt=np.full(2, -1, np.int32),
                     list_level=np.zeros(2, np.uint8), pt_nobs=None, pt_bad=None, obs_off=None, obs_kf=None, obs_level=None, obs_bad=None)
    got = K.walk(ctx, no_points)
    assert got["verdict"].tolist() == [0] and got["n_mps"].tolist() == [0]


@pytest.mark.gpu
def test_two_candidates_the_chain(ctx, K):
    got = _check(ctx, K, chain_scene(), "chain", 0.5)
    assert got["verdict"].tolist() == [CULLED, 0] and got["pt_nobs_out"].tolist() == [3] and got["n_reeval"] == 1


@pytest.mark.gpu
def test_forty_candidates_with_lists_of_three_hundred(ctx, K):
    sc = K.make_scene(seed=31, n_cand=40, n_out=14, n_pt=5400, window=16)
    assert np.diff(sc["list_off"]).min() > 256           # more than one workgroup of the first kernel per candidate
    got = _check(ctx, K, sc, "forty", 0.9)
    assert (got["verdict"] == CULLED).sum() >= 3 and (got["verdict"] == REDUNDANT_NOT_ERASED).any() and got["n_reeval"] > 0


@pytest.mark.gpu
def test_lists_longer_than_either_workgroup_strides(ctx, K):
    sc = K.make_scene(seed=24, n_cand=3, n_out=4, n_pt=2500, window=7, fine_obs=(5, 7), skip_frac=0, not_erase_frac=0)
    assert np.diff(sc["list_off"]).min() > 8 * 256       # beyond the first kernel's workgroups per candidate and the second kernel's 1024 lanes
    got = _check(ctx, K, sc, "long lists", 0.5)
    assert got["verdict"][0] == CULLED and got["n_reeval"] == 2


@pytest.mark.gpu
def test_three_hundred_candidates(ctx, K):
    sc = K.make_scene(seed=25, n_cand=300, n_out=60, n_pt=1500)
    got = _check(ctx, K, sc, "three hundred", 0.9)
    culled = np.flatnonzero(got["verdict"] == CULLED)
    assert culled.size >= 3 and culled.max() >= 256 and np.unique(culled // 32).size >= 4     # several words of the erased bitmask


@pytest.mark.gpu
def test_points_with_seventy_to_a_hundred_and_thirty_observers(ctx, K):
    sc = K.make_scene(seed=26, n_cand=60, n_out=100, n_pt=150, fine_frac=0.5, fine_obs=(70, 130), max_obs=130, window=150, mean_obs=5.0)
    n = np.diff(sc["obs_off"])
    assert (n > 64).sum() > 40 and n.max() > 128 and (n <= 64).sum() > 40       # a lane per slot and a wave per slot, the latter with two and three steps
    for thres in (0.4, 0.9):
        _check(ctx, K, sc, "wide points", thres)


@pytest.mark.gpu
def test_most_candidates_are_evaluated_again(ctx, K):
    sc = random_scene(K, 1)
    got = _check(ctx, K, sc, ("random", 1), 0.5)
    assert got["n_reeval"] > sc["n_cand"] / 2 and (got["verdict"] == CULLED).sum() >= 3


@pytest.mark.gpu
def test_no_erasure_no_second_evaluation(ctx, K):
    sc = K.make_scene(seed=27, n_cand=14, n_out=6, n_pt=260, fine_frac=0.3)
    got = _check(ctx, K, sc, "sparse", 0.98)
    assert not (got["verdict"] == CULLED).any() and got["n_reeval"] == 0 and got["n_mps"].max() > 0
    assert np.array_equal(got["pt_nobs_out"], sc["pt_nobs"]) and np.array_equal(got["pt_gone"], sc["pt_bad"])


@pytest.mark.gpu
def test_repeated_calls_on_one_context(ctx, K):
    sc, other = random_scene(K, 2), random_scene(K, 3)
    first = K.walk(ctx, sc, thres=0.5)
    K.walk(ctx, other, thres=0.9)
    again = K.walk(ctx, sc, thres=0.5)
    assert_same(again, first, "a second call")
    assert again["n_reeval"] == first["n_reeval"]


@pytest.mark.gpu
def test_two_contexts_on_two_threads(ctx, K):
    from ccm_slam_amd._lib import Context
    scenes = [random_scene(K, 4), K.make_scene(seed=28, n_cand=40, n_out=14, n_pt=1200)]
    solo = [K.walk(ctx, sc, thres=0.5) for sc in scenes]
    out, gate = [None, None], threading.Barrier(2)

    def run(i):
        c = Context(0)
        try:
            gate.wait()
            out[i] = [K.walk(c, scenes[i], thres=0.5) for _ in range(5)]
        finally:
            c.close()

    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(2):
        assert out[i] is not None
        for got in out[i]:
            assert_same(got, solo[i], f"thread {i}")


@pytest.mark.gpu
def test_bad_arguments_return_the_error_code(ctx, K):
    sc = random_scene(K, 0)
    good = K.walk(ctx, sc)
    for what, rc in bad_calls(K, K._device(), (ctx.handle,), sc):
        assert rc == -1, what
    with pytest.raises(K.CcmError):
        K.walk(ctx, dict(sc, n_all=1))
    assert_same(K.walk(ctx, sc), good, "after the refused calls")


@pytest.mark.gpu
def test_mirror_on_the_device_equals_the_mirror_on_the_host(ctx, K):
    sc = random_scene(K, 3)
    dev, host = K.KeyFrameCullingBatch(sc, thres=0.5, device=0), K.KeyFrameCullingBatch(sc, thres=0.5)
    rd, rh = dev.results(), host.results()
    assert_same(rd, rh, "mirror")
    assert rd["n_reeval"] == rh["n_reeval"] and dev.culled().tolist() == host.culled().tolist() and dev.points_gone().tolist() == host.points_gone().tolist()
    assert dev.culled().size > 0 and dev.points_gone().size > 0
    dev.close(); host.close()
