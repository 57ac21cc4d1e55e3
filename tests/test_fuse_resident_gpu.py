"""GPU: ccm_fuse_sim3_eval_resident and ccm_fuse_pose_eval_resident against the existing stateless device calls and the host evaluator, bit for
bit: one pair, no pair, no keyframe, a keyframe without features, tiles and waves that are full, one short and one over, the 8-keyframe scene, windows a lane walks
alone and windows the wave takes, job lists with shared keyframes and overlapping ranges, a device-built grid against a supplied one, permuted and repeated keys,
a key that is not live, the mirrors' walks on the device, and two threads on one store."""
import copy
import threading

import numpy as np
import pytest

import oracle
from ccm_slam_amd import fuse_pose as fp, fuse_sim3 as fs, kfstore as ks, synth
from fuse_pose_cases import CALLS, CURRENT, N_KF, fan_out_scene
from fuse_pose_cases import disc as pose_disc
from fuse_sim3_cases import DISC_SIZES, disc, planted, scene_from_frames
from kfstore_cases import lockstep_pose, lockstep_sim3, same_result
from test_fuse_pose_cpu import JOB_LISTS, N_PREDICTED, mirror_scene
from test_fuse_sim3_cpu import KINDS
from test_kfstore_cpu import ORDERS, POSE_ORDERS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    o = oracle.OrbOracle(1000)
    out = [o.extract(synth.gen_image(1000, t)) for t in (0, 1)]
    o.close()
    return out


@pytest.fixture(scope="module")
def mixed(ctx, frames):
    """the 8-keyframe scene, the host evaluator's answer, and a device store with its keyframes under 100 .. 107 (grids built on the device)"""
    sc = scene_from_frames(frames, KINDS)[0]
    store = ks.KeyFrameStore(ctx, 24, 1100)
    store.add_scene(range(100, 108), sc)
    yield sc, fs.fuse_sim3_eval_host(sc, want_uv=True), store
    store.close()


@pytest.fixture(scope="module")
def fan(ctx, frames):
    sc, info = fan_out_scene(frames)
    store = ks.KeyFrameStore(ctx, 12, 1100)
    store.add_scene(range(200, 200 + N_KF), sc)
    yield sc, info, store
    store.close()


def both(ctx, store, keys, sub, tag):
    """the resident call against the stateless device call and the host evaluator, with uv and without"""
    want = fs.fuse_sim3_eval_host(sub, want_uv=True)
    got = ks.fuse_sim3_eval_resident(ctx, store, keys, sub, want_uv=True)
    same_result(got, want, tag)
    same_result(got, fs.fuse_sim3_eval(ctx, sub, want_uv=True), (tag, "stateless"))
    bare = ks.fuse_sim3_eval_resident(ctx, store, keys, sub)
    assert "uv" not in bare
    same_result(bare, want, (tag, "without uv"), keys=("table", "n_valid", "n_hit"))
    return got


def test_one_pair_no_pair_no_keyframe_and_a_keyframe_without_features(ctx, mixed):
    sc, _, store = mixed
    for kfs, P in (([0], 1), ([0], 0), ([], 7), ([], 0), ([0, 5], 1)):
        got = both(ctx, store, [100 + k for k in kfs], sc.subset(kfs, P), (kfs, P))
        assert got["table"].shape == (len(kfs), P)
    pl = planted()
    ps = pl.scene()
    st = ks.KeyFrameStore(ctx, ps.K, 8)
    try:
        st.add_scene(range(ps.K), ps, grid=True)      # the planted scene has a hand-made grid among its keyframes
        assert st.get(0)["n"] == 0
        got = both(ctx, st, list(range(ps.K)), ps, "planted")
        pl.check(got["table"], "resident")
        assert got["n_hit"][0] == 0 and got["n_valid"][0] > 0
    finally:
        st.close()


def test_tile_and_wave_edges(ctx, mixed):
    sc, want, store = mixed
    near = [k for k, c in enumerate(KINDS) if c == "n"]
    for K in (1, 2, 3):
        for P in (63, 64, 65, 255, 256, 257):
            got = both(ctx, store, [100 + k for k in near[:K]], sc.subset(near[:K], P), (K, P))
            assert np.array_equal(got["table"], want["table"][near[:K], :P]) and got["n_hit"].min() > 0


@pytest.mark.parametrize("name", ["all"] + list(ORDERS))
def test_the_eight_keyframe_scene_in_any_order_of_keys(ctx, mixed, name):
    sc, want, store = mixed
    order = list(range(8)) if name == "all" else ORDERS[name]
    got = both(ctx, store, [100 + k for k in order], sc.subset(order), name)
    assert np.array_equal(got["table"], want["table"][order]) and got["n_hit"].max() > 1000


def test_windows_on_both_sides_of_the_wave_switch(ctx):
    for pl, ev_host, n_disc in ((disc(), fs.fuse_sim3_eval_host, 7), (pose_disc(), fp.fuse_pose_eval_host, 7)):
        sc = pl.scene()
        want = ev_host(sc, want_uv=True, want_cand=True)
        nc = want["n_cand"].reshape(sc.K, sc.P)
        assert nc[:, n_disc].tolist() == list(DISC_SIZES) and nc.max() > 256      # on the host first: 0 .. 64 stay with the lane, 65, 70 and 300 go to the wave
        st = ks.KeyFrameStore(ctx, sc.K, 304)
        try:
            st.add_scene(range(sc.K), sc)
            if isinstance(sc, fs.Scene):
                both(ctx, st, list(range(sc.K)), sc, "disc")
            else:
                got = ks.fuse_pose_eval_resident(ctx, st, list(range(sc.K)), sc, want_uv=True)
                same_result(got, want, "pose disc")
                same_result(got, fp.fuse_pose_eval(ctx, sc, want_uv=True), "pose disc, stateless")
        finally:
            st.close()


@pytest.mark.parametrize("order_name", list(POSE_ORDERS))
@pytest.mark.parametrize("name", list(JOB_LISTS))
def test_pose_job_lists_with_shared_keyframes_and_overlapping_ranges(ctx, fan, name, order_name):
    sc, info, store = fan
    order = POSE_ORDERS[order_name]
    place = lambda k, j: [i for i, o in enumerate(order) if o == k][-(j % 2)]
    sub = sc.subset(order, jobs=[(place(k, j), p0, n) for j, (k, p0, n) in enumerate(JOB_LISTS[name])])
    keys = [200 + k for k in order]
    want = fp.fuse_pose_eval_host(sub, want_uv=True)
    got = ks.fuse_pose_eval_resident(ctx, store, keys, sub, want_uv=True)
    same_result(got, want, (name, order_name))
    same_result(got, fp.fuse_pose_eval(ctx, sub, want_uv=True), (name, order_name, "stateless"))
    bare = ks.fuse_pose_eval_resident(ctx, store, keys, sub)
    assert "uv" not in bare
    same_result(bare, want, (name, "without uv"), keys=("table", "n_valid", "n_hit"))
    assert got["n_hit"].sum() > 100


def test_pose_empty_calls(ctx, fan):
    sc, info, store = fan
    for kfs, P, jobs in (([], 30, []), ([], 0, []), ([0, 1], 0, []), ([0, 1], 0, [(1, 0, 0)]), ([0, 1], 30, []), ([0], 30, [(0, 30, 0), (0, 0, 0)]), ([2], 1, [(0, 0, 1)])):
        sub = sc.subset(kfs, P, jobs)
        got = ks.fuse_pose_eval_resident(ctx, store, [200 + k for k in kfs], sub, want_uv=True)
        same_result(got, fp.fuse_pose_eval_host(sub, want_uv=True), (kfs, P, jobs))


def test_a_device_built_grid_against_a_supplied_one(ctx, mixed):
    sc, want, built = mixed
    given = ks.KeyFrameStore(ctx, 8, 1100)
    try:
        given.add_scene(range(8), sc, grid=True)
        for k in range(8):
            a, b = built.get(100 + k), given.get(k)
            assert a["n_in"] == b["n_in"] == a["n"] and np.array_equal(a["cell_off"], b["cell_off"]) and np.array_equal(a["cell_idx"], b["cell_idx"])
        same_result(ks.fuse_sim3_eval_resident(ctx, given, range(8), sc, want_uv=True), want, "a supplied grid")
        same_result(ks.fuse_sim3_eval_resident(ctx, built, range(100, 108), sc, want_uv=True), want, "a device-built grid")
    finally:
        given.close()


def test_a_key_that_is_not_live_is_refused_with_nothing_launched_and_the_next_call_is_correct(ctx, mixed, fan):
    sc, want, store = mixed
    sub = sc.subset([1, 2], 300)
    table = np.full(600, 0xDEADBEEF, np.uint32); nv = np.full(2, -5, np.int32); nh = np.full(2, -5, np.int32)
    for keys in ([101, 999], [999, 101]):
        k, args = ks._sim3_args(keys, sub)
        assert ks._dev().ccm_fuse_sim3_eval_resident(ctx.handle, store.raw, *args, ks._p(table), ks._p(nv), ks._p(nh), None) == -1      # CCM_E_ARG
        assert (table == 0xDEADBEEF).all() and (nv == -5).all()
    store.add_scene([150], sc, [3])
    same_result(ks.fuse_sim3_eval_resident(ctx, store, [150, 102], sc.subset([3, 2], 300)), fs.fuse_sim3_eval_host(sc.subset([3, 2], 300)), "before the erase")
    store.erase(150)
    with pytest.raises(ks.CcmError):
        ks.fuse_sim3_eval_resident(ctx, store, [150, 102], sc.subset([3, 2], 300))
    for over in (dict(th=0.0), dict(nlevels=0), dict(nlevels=17)):
        b = copy.copy(sub)
        for kk, v in over.items():
            setattr(b, kk, v)
        with pytest.raises(ks.CcmError):
            ks.fuse_sim3_eval_resident(ctx, store, [101, 102], b)
    with pytest.raises(ks.CcmError):
        k, args = ks._sim3_args([101, 102], sub)
        ks.check(ks._dev().ccm_fuse_sim3_eval_resident(ctx.handle, None, *args, ks._p(table), ks._p(nv), ks._p(nh), None), ctx.handle)      # a NULL store
    same_result(ks.fuse_sim3_eval_resident(ctx, store, [101, 102], sub, want_uv=True), fs.fuse_sim3_eval_host(sub, want_uv=True), "after the refusals")
    psc, info, pstore = fan
    for keys, jobs in (([200, 555], [(0, 0, 10)]), ([200, 201], [(2, 0, 10)]), ([200, 201], [(0, 7495, 6)])):
        with pytest.raises(ks.CcmError):
            ks.fuse_pose_eval_resident(ctx, pstore, keys, psc.subset([0, 1], jobs=jobs))
    ok = psc.subset([0, 1], jobs=[(1, 5, 300), (0, 0, 10)])
    same_result(ks.fuse_pose_eval_resident(ctx, pstore, [200, 201], ok, want_uv=True), fp.fuse_pose_eval_host(ok, want_uv=True), "pose, after the refusals")


def test_mirrors_on_the_device_walk_like_the_mirrors_on_a_scene(ctx, frames, mixed, fan):
    sc, want, _ = mixed
    store = ks.KeyFrameStore(ctx, 10, 1100)
    try:
        keys = list(range(40, 48))
        store.add_scene(keys, sc)
        old = fs.SearchAndFuseBatch(None, sc); new = ks.SearchAndFuseBatchResident(store, keys, sc)
        try:
            assert np.array_equal(new.table()["table"], want["table"])

            def between(k):
                if k == 2:
                    store.erase(45); store.erase(43)
            which = [k % 2 for k in range(sc.K)]
            assert lockstep_sim3(old, new, sc.K, sc.P, sc.pt_desc, lambda k: frames[which[k]][1], between) > 100
        finally:
            old.close(); new.close()
        store.clear()
        psc, info, _ = fan
        ms = mirror_scene(psc, info)
        keys = list(range(300, 300 + N_KF))
        store.add_scene(keys, ms)
        old = fp.SearchInNeighborsBatch(None, ms, CALLS, CURRENT, info["n1"]); new = ks.SearchInNeighborsBatchResident(store, keys, ms, CALLS, CURRENT, info["n1"])
        try:
            assert np.array_equal(old.table()["table"], new.table()["table"])

            def between(c):
                if c == 3:
                    store.erase(300 + CALLS[5]); store.erase(300 + CURRENT)
            cand, slot, skip_c, desc_now, fresh = lockstep_pose(old, new, CALLS, info["n1"], N_PREDICTED, info["n2"], psc, frames[0][1], between)
            ra, rb = old.resolve_current(slot, skip_c, desc_now, fresh), new.resolve_current(slot, skip_c, desc_now, fresh)
            assert ra[0] == rb[0] > 300 and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
            assert old.n_reeval() == new.n_reeval() > 100 and old.n_unpredicted() == new.n_unpredicted() > 20
        finally:
            old.close(); new.close()
    finally:
        store.close()


def test_two_threads_two_contexts_one_store(mixed):
    """one thread makes 20 resident calls on keys it owns while the other adds and erases other keys, a bounded number of times; every answer equals the solo one"""
    from ccm_slam_amd._lib import Context
    sc, want, store = mixed
    sub = sc.subset([0, 3, 4, 1], 1200)
    keys = [100, 103, 104, 101]
    solo = fs.fuse_sim3_eval_host(sub, want_uv=True)
    errs = []; done = threading.Event(); rounds = []

    def reader():
        try:
            c = Context(0)
            try:
                same_result(ks.fuse_sim3_eval_resident(c, store, keys, sub, want_uv=True), solo, "solo")
                for i in range(20):
                    same_result(ks.fuse_sim3_eval_resident(c, store, keys, sub, want_uv=True), solo, f"call {i}")
            finally:
                c.close()
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
        finally:
            done.set()

    def writer():
        try:
            n = 0
            for i in range(60):      # bounded, whatever the reader does
                store.add_scene([500 + i % 3, 600 + i % 3], sc, [i % 8, (i + 3) % 8])
                store.erase(500 + i % 3); store.erase(600 + i % 3)
                n += 1
                if done.is_set() and n >= 5:
                    break
            rounds.append(n)
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=reader), threading.Thread(target=writer)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert rounds and rounds[0] >= 5 and store.count()[0] == 8
