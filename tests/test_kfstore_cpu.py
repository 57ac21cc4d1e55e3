"""The keyframe feature store on the CPU: the host-only cslam::KeyFrameStore, whose grid is csrc/kfstore_math.h compiled by g++ — the host evaluator
of the device's grid kernel — against kfstore.build_grid_keyframe, the literal Python replay of KeyFrame::AssignFeaturesToGrid / PosInGrid; the store's bookkeeping
and every refusal; the resident host evaluation against fuse_sim3_eval_host / fuse_pose_eval_host on the same data; a keyframe with features outside the grid; the
mirrors' walks through the constructors that take a store.  Every comparison is exact: integers and f32 bit patterns."""
import copy

import numpy as np
import pytest

import oracle
import tests.test_ref_matcher as trm
from ccm_slam_amd import fuse_pose as fp, fuse_sim3 as fs, kfstore as ks, synth
from fuse_pose_cases import CALLS, CURRENT, N_KF, fan_out_scene
from fuse_sim3_cases import scene_from_frames
from kfstore_cases import (EIGHTH, add_one, bookkeeping_sequence, grid_cases, lockstep_pose, lockstep_sim3, planted_roundings, refusals, same_grid, same_result)
from test_fuse_pose_cpu import JOB_LISTS, N_PREDICTED, mirror_scene
from test_fuse_sim3_cpu import KINDS


@pytest.fixture(scope="module")
def frames():
    o = oracle.OrbOracle(1000)
    out = [o.extract(synth.gen_image(1000, t)) for t in (0, 1)]
    o.close()
    return out


@pytest.fixture(scope="module")
def mixed(frames):
    """the 8-keyframe scene, the host evaluator's answer and a host-only store that holds its keyframes under the keys 100 .. 107 (grids built by the store)"""
    sc = scene_from_frames(frames, KINDS)[0]
    store = ks.KeyFrameStore(None, 16, 1100)
    store.add_scene(range(100, 108), sc)
    return sc, fs.fuse_sim3_eval_host(sc, want_uv=True), store


@pytest.fixture(scope="module")
def fan(frames):
    sc, info = fan_out_scene(frames)
    store = ks.KeyFrameStore(None, 16, 1100)
    store.add_scene(range(200, 200 + N_KF), sc)
    return sc, info, store


@pytest.mark.parametrize("case", grid_cases(), ids=lambda c: c[0])
def test_host_grid_equals_the_replay_of_assign_features_to_grid(case):
    name, xy, rec = case
    store = ks.KeyFrameStore(None, 2, max(len(xy), 1))
    add_one(store, 5, xy, rec)
    same_grid(store.get(5), xy, rec, name)
    store.close()


def test_planted_roundings_have_their_known_cells():
    xy, cells = planted_roundings()
    # t = -0.5 is out, -0.49.. is cell 0, 0.5 -> 1, 73.5 -> 74, 74.5 is out (x); the same in y with 46.5 -> 47 and 47.5 out; y = 8 is row 1, x = 8 column 1
    assert cells[:12].tolist() == [-1, -1, 1, 1, 49, 49, 73 * 48 + 1, 74 * 48 + 1, 74 * 48 + 1, 74 * 48 + 1, -1, -1]
    assert cells[12:].tolist() == [-1, -1, 48, 48, 49, 49, 48 + 46, 48 + 47, 48 + 47, 48 + 47, -1, -1]
    off, idx = ks.build_grid_keyframe(xy, EIGHTH)
    cell_of = -np.ones(len(xy), int)
    for c in range(fs.CELLS):
        cell_of[idx[off[c]:off[c + 1]]] = c
    assert np.array_equal(cell_of, cells)
    store = ks.KeyFrameStore(None, 1, 64)
    add_one(store, 1, xy, EIGHTH)
    got = store.get(1)
    assert np.array_equal(got["cell_off"], off) and np.array_equal(got["cell_idx"], idx) and got["n_in"] == int((cells >= 0).sum())


def test_frame_rule_and_keyframe_rule_agree_on_the_scenes_bounds(frames, mixed, fan):
    """a pre-assertion on the two references alone: with integral bounds build_grid (Frame::PosInGrid on the float bounds) and build_grid_keyframe
    (KeyFrame::PosInGrid on the int bounds) give the same grid for every keyframe of the scenes used below"""
    assert tuple(trm.BOUNDS) == tuple(fs.BOUNDS) and all(float(b) == int(b) for b in fs.BOUNDS)
    for sc in (mixed[0], fan[0], fs.make_scene(2, 4, n_feat=1000, seed=0)):
        for k in range(sc.K):
            a, b = int(sc.feat_off[k]), int(sc.feat_off[k + 1])
            xy = sc.feat_xy[2 * a:2 * b].reshape(-1, 2)
            off_f, idx_f = fs.build_grid(xy, fs.BOUNDS)
            off_k, idx_k = ks.build_grid_keyframe(xy, sc.rec[10 * k:10 * k + 10])
            assert np.array_equal(off_f, off_k) and np.array_equal(idx_f, idx_k), k
            assert np.array_equal(off_f, sc.cell_off[k * (fs.CELLS + 1):(k + 1) * (fs.CELLS + 1)]) and np.array_equal(idx_f, sc.cell_idx[a:b]), k


def test_bookkeeping_slot_reuse_and_every_refusal():
    store = ks.KeyFrameStore(None, 4, 256)
    bookkeeping_sequence(store)
    refusals(store)
    store.clear()
    assert store.count() == (0, 4)
    with pytest.raises(ks.StoreError):
        store.get(1)
    bookkeeping_sequence(store)      # and again in the cleared store
    for bad in ((0, 10), (1, 0), (1, 65536), (40000, 65535)):
        with pytest.raises(ks.CcmError):
            ks.KeyFrameStore(None, *bad)
    ks.KeyFrameStore(None, 1, 65535).close()


ORDERS = {"another order": [5, 0, 7, 2, 1, 6, 3, 4], "one key twice": [3, 1, 3, 6], "one key": [4]}


@pytest.mark.parametrize("name", list(ORDERS))
def test_resident_sim3_host_evaluation_equals_the_stateless_one(mixed, name):
    sc, want, store = mixed
    order = ORDERS[name]
    sub = sc.subset(order)
    got = ks.fuse_sim3_eval_resident_host(store, [100 + k for k in order], sub, want_uv=True)
    same_result(got, fs.fuse_sim3_eval_host(sub, want_uv=True), name)
    assert np.array_equal(got["table"], want["table"][order]) and got["n_hit"].max() > 1000      # (the far keyframes hit little or nothing)
    bare = ks.fuse_sim3_eval_resident_host(store, [100 + k for k in order], sub)
    assert "uv" not in bare and np.array_equal(bare["table"], got["table"])


def test_resident_host_evaluation_refuses_what_the_stateless_one_refuses_and_a_key_that_is_not_live(mixed, fan):
    sc, _, store = mixed
    sub = sc.subset([0, 1], 50)
    with pytest.raises(ks.CcmError):
        ks.fuse_sim3_eval_resident_host(store, [100, 999], sub)
    for over in (dict(th=0.0), dict(th=float("nan")), dict(nlevels=0), dict(nlevels=17)):
        b = copy.copy(sub)
        for k, v in over.items():
            setattr(b, k, v)
        with pytest.raises(ks.CcmError):
            ks.fuse_sim3_eval_resident_host(store, [100, 101], b)
    assert ks.fuse_sim3_eval_resident_host(store, [], sc.subset([], 50))["table"].size == 0
    assert ks.fuse_sim3_eval_resident_host(store, [100], sc.subset([0], 0))["table"].shape == (1, 0)
    psc, info, pstore = fan
    for jobs in ([(2, 0, 10)], [(0, 0, 10), (0, 7495, 6)], [(0, -1, 3)]):      # a keyframe outside the keys, a job beyond P, a negative start
        with pytest.raises(ks.CcmError):
            ks.fuse_pose_eval_resident_host(pstore, [200, 201], psc.subset([0, 1], jobs=jobs))
    with pytest.raises(ks.CcmError):
        ks.fuse_pose_eval_resident_host(pstore, [200, 555], psc.subset([0, 1], jobs=[(0, 0, 10)]))


POSE_ORDERS = {"another order": [3, 1, 5, 0, 8, 2, 4, 6, 7], "one key twice": [3, 1, 5, 1, 0, 2, 4, 6, 7, 8, 5]}


@pytest.mark.parametrize("order_name", list(POSE_ORDERS))
@pytest.mark.parametrize("name", list(JOB_LISTS))
def test_resident_pose_host_evaluation_equals_the_stateless_one(fan, name, order_name):
    sc, info, store = fan
    order = POSE_ORDERS[order_name]
    # a job's keyframe in the new order; a keyframe listed twice is taken at its first place by the even jobs and at its last place by the odd ones
    place = lambda k, j: [i for i, o in enumerate(order) if o == k][-(j % 2)]
    jobs = [(place(k, j), p0, n) for j, (k, p0, n) in enumerate(JOB_LISTS[name])]
    sub = sc.subset(order, jobs=jobs)
    got = ks.fuse_pose_eval_resident_host(store, [200 + k for k in order], sub, want_uv=True)
    same_result(got, fp.fuse_pose_eval_host(sub, want_uv=True), (name, order_name))
    same_result(got, fp.fuse_pose_eval_host(sc.subset(jobs=JOB_LISTS[name])), (name, order_name, "the scene's own order"))
    assert got["n_hit"].sum() > 100


def test_a_keyframe_with_features_outside_the_grid(mixed):
    """the resident answer on a keyframe some of whose keypoints lie outside the grid (undistortion can push them there) equals the stateless answer on the scene
    with those keypoints removed, after renumbering the kept features"""
    sc, _, _ = mixed
    one = sc.subset([0])
    n = int(one.feat_off[1])
    xy = one.feat_xy.reshape(-1, 2).copy()
    rng = np.random.default_rng(12)
    out = np.sort(rng.choice(n, 60, replace=False))
    xy[out[0::3], 0] = 756.5 + rng.uniform(0, 30, out[0::3].size)      # t > 75.4: column 75 and beyond
    xy[out[1::3], 1] = -6.0 - rng.uniform(0, 30, out[1::3].size)        # t < -0.5
    xy[out[2::3]] = np.nan
    kept = np.setdiff1d(np.arange(n), out)
    store = ks.KeyFrameStore(None, 2, 1100)
    store.add([7], one.rec, [0, n], xy, one.feat_octave, one.feat_desc)
    g = store.get(7)
    assert (g["n"], g["n_in"]) == (n, n - 60) and not np.isin(g["cell_idx"], out).any()
    got = ks.fuse_sim3_eval_resident_host(store, [7], one, want_uv=True)
    kxy = xy[kept]
    grid = fs.build_grid(kxy, fs.BOUNDS)
    removed = fs.Scene(one.rec, [0, kept.size], kxy, one.feat_octave[kept], one.feat_desc.reshape(-1, 32)[kept], grid[0], grid[1], one.Scw, one.scale_factors, one.log_sf,
                       one.th, one.pos, one.normal, one.min_dist, one.max_dist, one.pt_desc)
    want = fs.fuse_sim3_eval_host(removed, want_uv=True)
    tg, tw = fs.unpack_table(got["table"]), fs.unpack_table(want["table"])
    for k in ("status", "dist", "level"):
        assert np.array_equal(tg[k], tw[k]), k
    assert np.array_equal(tg["idx"], np.where(tw["idx"] >= 0, kept[np.maximum(tw["idx"], 0)], -1))
    assert np.array_equal(got["uv"].view(np.uint32), want["uv"].view(np.uint32)) and np.array_equal(got["n_hit"], want["n_hit"]) and want["n_hit"][0] > 500
    assert (fs.unpack_table(fs.fuse_sim3_eval_host(one)["table"])["idx"] != tg["idx"]).any()      # the moved keypoints mattered


def test_sim3_mirror_on_a_store_walks_like_the_mirror_on_a_scene(frames, mixed):
    sc, want, _ = mixed
    store = ks.KeyFrameStore(None, 8, 1100)
    keys = list(range(40, 48))
    store.add_scene(keys, sc)
    old = fs.SearchAndFuseBatch(None, sc)
    new = ks.SearchAndFuseBatchResident(store, keys, sc)
    try:
        tb = new.table()
        assert np.array_equal(tb["table"], want["table"]) and np.array_equal(tb["n_hit"], want["n_hit"]) and np.array_equal(tb["n_valid"], want["n_valid"])

        def between(k):
            if k == 2:      # keyframes still to be resolved leave the store: the batch holds their shadows
                store.erase(45); store.erase(43)
                assert store.count() == (6, 2)
            if k == 4:
                store.clear()
        which = [k % 2 for k in range(sc.K)]
        n = lockstep_sim3(old, new, sc.K, sc.P, sc.pt_desc, lambda k: frames[which[k]][1], between)
        assert n > 100
    finally:
        old.close(); new.close()
    with pytest.raises(ks.CcmError):
        ks.SearchAndFuseBatchResident(store, keys, sc)      # the keys are gone


def test_pose_mirror_on_a_store_walks_like_the_mirror_on_a_scene(frames, fan):
    sc, info, _ = fan
    ms = mirror_scene(sc, info)
    store = ks.KeyFrameStore(None, 9, 1100)
    keys = list(range(300, 300 + N_KF))
    store.add_scene(keys, ms)
    old = fp.SearchInNeighborsBatch(None, ms, CALLS, CURRENT, info["n1"])
    new = ks.SearchInNeighborsBatchResident(store, keys, ms, CALLS, CURRENT, info["n1"])
    try:
        ta, tb = old.table(), new.table()
        assert np.array_equal(ta["table"], tb["table"]) and np.array_equal(ta["n_hit"], tb["n_hit"]) and np.array_equal(ta["n_valid"], tb["n_valid"])

        def between(c):
            if c == 3:
                store.erase(300 + CALLS[5]); store.erase(300 + CURRENT)
        cand, slot, skip_c, desc_now, fresh = lockstep_pose(old, new, CALLS, info["n1"], N_PREDICTED, info["n2"], sc, frames[0][1], between)
        ra, rb = old.resolve_current(slot, skip_c, desc_now, fresh), new.resolve_current(slot, skip_c, desc_now, fresh)
        assert ra[0] == rb[0] > 300 and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
        assert old.n_reeval() == new.n_reeval() > 100 and old.n_unpredicted() == new.n_unpredicted() > 20
    finally:
        old.close(); new.close()
