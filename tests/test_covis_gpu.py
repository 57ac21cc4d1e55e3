"""GPU: ccm_covis_update against the host evaluator of the same header and against the sequential replay of test_covis_cpu.py, array for array (exact integer
equality): the sizes of a loop and of one agent's map, rows and lists that cross wave and workgroup boundaries, several histogram windows through the test hook,
the edge shapes, two walk orders, repeated calls, a capacity that is too small and every CCM_E_ARG case."""
import numpy as np
import pytest

from test_covis_cpu import CHANGED, EMPTY, FALLBACK, assert_same, bad_arguments, mixed_scene, replay_arrays, sparse_scene, state_by_old_index, walks


@pytest.fixture(scope="module")
def V():
    from ccm_slam_amd import covis
    return covis


def _check(ctx, V, sc, tag, th=15, **kw):
    """device == host evaluator == replay; returns the device's arrays"""
    got = V.update(ctx, sc, th=th, **kw)
    assert_same(got, V.update_host(sc, th=th), f"{tag}: device against the host evaluator")
    assert_same(got, replay_arrays(sc, th=th, tag=tag), f"{tag}: device against the replay")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["loop", "agent"])
def test_device_matches_host_and_replay(ctx, V, size):
    n_kf, n_pt = V.SIZES[size]
    sc = V.make_scene(seed=100 + n_kf, n_kf=n_kf, n_pt=n_pt)
    assert np.diff(sc["list_off"]).max() > 256                      # lists longer than the workgroup: the stride loop
    got = _check(ctx, V, sc, size)
    assert (got["ord_w"] >= 15).any()
    if size == "loop":
        assert_same(V.update(ctx, sc), got, "a second call on the same context")
        # a capacity that is too small: the sizes come back, the second call is complete
        rc, _, needed = V.call(V._device(False), (ctx.handle,), sc, 15, 16)
        assert rc == 0 and needed[0] == got["col"].size and needed[1] == -1 and needed[2] == -1
        rc, _, needed = V.call(V._device(False), (ctx.handle,), sc, 15, int(got["col"].size))
        assert rc == 0 and needed.tolist() == [got["col"].size, got["fw_col"].size, got["ord_kf"].size]
        again = V.update(ctx, sc, cap=16)
        assert again["calls"] >= 2
        assert_same(again, got, "after growing the capacity")


@pytest.mark.gpu
def test_rows_and_lists_across_waves(ctx, V):
    # twelve keyframes that each see nearly all of 311 others: count rows, final rows and (with th = 1) ordered lists of more than 256 entries
    sc = V.make_scene(seed=11, n_kf=12, n_out=300, n_pt=3000, window=312, mean_obs=20.0, max_obs=30, stale_frac=0.05, dup_frac=0.02)
    got = _check(ctx, V, sc, "wide", th=1)
    assert np.diff(got["row_off"]).min() > 256 and np.diff(got["ord_off"]).min() > 256 and (got["flags"] & CHANGED).any()
    got = _check(ctx, V, sc, "wide", th=15)
    assert (np.diff(got["ord_off"]) < np.diff(got["row_off"])).any() and (got["ord_w"] >= 15).any()


@pytest.mark.gpu
def test_several_histogram_windows(ctx, V):
    # the test hook's window holds 64 keyframe indices: 209 = three windows and 17
    sc = V.make_scene(seed=12, n_kf=150, n_out=59, n_pt=2500, window=120, mean_obs=8.0, stale_frac=0.05, dup_frac=0.02)
    assert sc["n_all"] == 3 * 64 + 17
    for th in (15, 1):
        got = V.update(ctx, sc, th=th, small_window=True)
        assert_same(got, replay_arrays(sc, th=th, tag="windows"), f"small window, th {th}")
        assert_same(got, V.update(ctx, sc, th=th), f"small window against the product's, th {th}")
    assert (got["col"] >= 192).any() and (got["col"] < 64).any()


@pytest.mark.gpu
def test_edge_shapes(ctx, V):
    one = V.make_scene(seed=13, n_kf=1, n_out=3, n_pt=40, window=4, mean_obs=3.0)
    got = _check(ctx, V, one, "one keyframe with observers")
    assert got["col"].size > 0 and (got["col"] >= 1).all()
    alone = V.make_scene(seed=14, n_kf=1, n_out=0, n_pt=40)
    got = _check(ctx, V, alone, "one keyframe alone")
    assert got["flags"].tolist() == [EMPTY] and got["col"].size == 0 and got["ord_kf"].size == 0
    closed = V.make_scene(seed=15, n_kf=30, n_out=0, n_pt=600, window=12, stale_frac=0.05)
    _check(ctx, V, closed, "no outside keyframe")
    sp = sparse_scene(V)
    got = _check(ctx, V, sp, ("sparse", 0))
    assert got["fw_col"].size > got["col"].size and (got["flags"] & FALLBACK).any()
    mx = mixed_scene(V)
    _check(ctx, V, mx, ("mixed", 0), th=1)
    got = _check(ctx, V, mx, ("mixed", 0), th=10**6)
    assert ((got["flags"] & (FALLBACK | EMPTY)) != 0).all()
    no_points = dict(mx, n_pt=0, obs_off=np.zeros(1, np.int32), obs_kf=np.zeros(0, np.int32), list_pt=np.full_like(mx["list_pt"], -1))
    got = V.update(ctx, no_points)
    assert (got["flags"] == EMPTY).all()


@pytest.mark.gpu
def test_two_walk_orders_differ_and_each_matches_its_replay(ctx, V):
    sc = mixed_scene(V)
    w = walks(sc["n_kf"])
    a, b = V.reorder(sc, w[0]), V.reorder(sc, w[1])
    ga, gb = _check(ctx, V, a, ("mixed", 0)), _check(ctx, V, b, ("mixed", 1))
    assert state_by_old_index(a, ga) != state_by_old_index(b, gb)


@pytest.mark.gpu
def test_mirror_on_the_device_equals_the_mirror_on_the_host(ctx, V):
    sc = sparse_scene(V)
    dev, host = V.CovisibilityBatch(sc, device=0), V.CovisibilityBatch(sc)
    rd, rh = dev.results(), host.results()
    assert_same(rd, rh)
    assert np.array_equal(rd["outside"], rh["outside"]) and np.array_equal(rd["outside"], replay_arrays(sc, tag=("sparse", 0))["outside"])
    for i in range(sc["n_kf"]):
        assert np.array_equal(dev.best_covisibles(i, 10), host.best_covisibles(i, 10))
    dev.close(); host.close()


@pytest.mark.gpu
def test_bad_arguments_return_the_error_code(ctx, V):
    sc = mixed_scene(V)
    fn = V._device(False)
    good = V.update(ctx, sc)
    for what, bad in bad_arguments(sc):
        rc, _, _ = V.call(fn, (ctx.handle,), bad, 15, 4096)
        assert rc == -1, what
    for th, cap in ((0, 4096), (15, -1)):
        assert V.call(fn, (ctx.handle,), sc, th, cap)[0] == -1
    with pytest.raises(V.CcmError):
        V.update(ctx, dict(sc, order_key=np.zeros(sc["n_all"], np.int32)))
    assert_same(V.update(ctx, sc), good, "after the refused calls")
