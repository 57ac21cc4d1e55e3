"""GPU: ccm_sim3_project_eval_resident and ccm_sim3_pair_eval_resident against the host evaluator, bit for bit (table, counters, uv present and
absent): no pair, one pair, tiles and waves that are full, one short and one over, no keyframe, a keyframe without features, job lists with an empty job, two jobs on
one keyframe and overlapping ranges, the planted masks and pairs, masked windows a lane walks alone and masked windows the wave takes, the two reference scenes, one key
twice with two masks, a device-built grid against a supplied one, a key that is not live, both mirrors on the device, and two threads on one store."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import oracle
import tests.test_ref_matcher as trm
from ccm_slam_amd import fuse_sim3 as fs, kfstore as ks, sim3_search as ss, synth
from fuse_sim3_cases import DISC_SIZES, disc, planted, scene_from_frames
from kfstore_cases import same_result
from sim3_search_cases import (expected_reeval, pair_all_points, pair_case, pair_keyframes, pair_planted, pair_sides, projection_case, projection_scene, ref_pair,
                               ref_projection)
from test_sim3_search_cpu import disc_masks, planted_mask_cases

pytestmark = pytest.mark.gpu
HAVE_REF = os.path.exists(trm.LIB)


@pytest.fixture(scope="module")
def frames():
    o = oracle.OrbOracle(1000)
    out = [o.extract(synth.gen_image(1000, t)) for t in (0, 1)]
    o.close()
    return out


@pytest.fixture(scope="module")
def four(ctx, frames):
    """four keyframes (two near, two far) under the keys 100 .. 103 with device-built grids, a random mask per keyframe, and the host evaluator's answer"""
    sc = scene_from_frames(frames, "nnff")[0]
    rng = np.random.default_rng(41)
    masks = [(rng.random(n) < 0.3).astype(np.uint8) for n in np.diff(sc.feat_off)]
    store = ks.KeyFrameStore(ctx, 8, 1100)
    store.add_scene(range(100, 104), sc)
    yield sc, masks, ss.project_eval_host(sc, masks, want_uv=True), store
    store.close()


@pytest.fixture(scope="module")
def pair(ctx, frames):
    """the pair scene: its two keyframes under 11 and 12 (supplied grids), every slot's point of both, and the host evaluator's answer"""
    p = pair_case(frames)
    kfs = pair_keyframes(p)
    store = ks.KeyFrameStore(ctx, 4, 1100)
    store.add_scene([11, 12], kfs, grid=True)
    ps = pair_all_points(p, kfs)
    yield p, kfs, ps, ss.pair_eval_host(ps, want_uv=True), store
    store.close()


def both_proj(ctx, store, keys, sub, masks, tag):
    want = ss.project_eval_host(sub, masks, want_uv=True)
    got = ss.project_eval_resident(ctx, store, keys, sub, masks, want_uv=True)
    same_result(got, want, tag)
    bare = ss.project_eval_resident(ctx, store, keys, sub, masks)
    assert "uv" not in bare
    same_result(bare, want, (tag, "without uv"))
    return got


def both_pair(ctx, store, keys, ps, tag):
    want = ss.pair_eval_host(ps, want_uv=True)
    got = ss.pair_eval_resident(ctx, store, keys, ps, want_uv=True)
    same_result(got, want, tag)
    bare = ss.pair_eval_resident(ctx, store, keys, ps)
    assert "uv" not in bare
    same_result(bare, want, (tag, "without uv"))
    return got


def test_projection_tile_and_wave_edges_no_keyframe_and_a_keyframe_without_features(ctx, four):
    sc, masks, want, store = four
    for kfs in ([0], [1, 2], [3, 0, 2]):
        for P in (0, 1, 63, 64, 65, 255, 256, 257):
            got = both_proj(ctx, store, [100 + k for k in kfs], sc.subset(kfs, P), [masks[k] for k in kfs], (kfs, P))
            assert got["table"].shape == (len(kfs), P) and np.array_equal(got["table"], want["table"][kfs, :P])
    assert want["n_hit"][:2].min() > 300
    for P in (0, 7):
        assert both_proj(ctx, store, [], sc.subset([], P), [], ("K = 0", P))["table"].size == 0


def test_planted_masks_and_masked_windows_on_both_sides_of_the_wave_switch(ctx):
    sc, masks, exp = planted_mask_cases()
    st = ks.KeyFrameStore(ctx, sc.K, 8)
    try:
        st.add_scene(range(sc.K), sc, grid=True)            # a hand-made grid among its keyframes; keyframe 0 has no features
        assert st.get(0)["n"] == 0
        t = fs.unpack_table(both_proj(ctx, st, list(range(sc.K)), sc, masks, "planted")["table"])
        for (k, i), (s_, idx, dist) in exp.items():
            assert (int(t["status"][k, i]), int(t["idx"][k, i]), int(t["dist"][k, i])) == (s_, idx, dist), (k, i)
    finally:
        st.close()
    sc = disc().scene()
    assert tuple(np.diff(sc.feat_off)) == DISC_SIZES
    nc = fs.fuse_sim3_eval_host(sc, want_cand=True)["n_cand"]
    assert nc[:, 7].tolist() == list(DISC_SIZES)            # 0 .. 64 stay with the lane, 65, 70 and 300 go to the wave
    st = ks.KeyFrameStore(ctx, sc.K, 304)
    try:
        st.add_scene(range(sc.K), sc)
        for masks in (disc_masks(sc), [1 - m for m in disc_masks(sc)], [np.ones_like(m) for m in disc_masks(sc)], None):
            got = both_proj(ctx, st, list(range(sc.K)), sc, masks if masks is not None else [None] * sc.K, "disc")
        same_result(got, fs.fuse_sim3_eval_host(sc, want_uv=True), "mask off = Fuse")
    finally:
        st.close()


def test_one_key_twice_with_two_masks_and_a_device_built_grid_against_a_supplied_one(ctx, four):
    sc, masks, want, built = four
    other = (1 - masks[1]).astype(np.uint8)
    got = both_proj(ctx, built, [101, 101, 100], sc.subset([1, 1, 0]), [masks[1], other, masks[0]], "one key twice")
    assert np.array_equal(got["table"][0], want["table"][1]) and not np.array_equal(got["table"][0], got["table"][1])
    given = ks.KeyFrameStore(ctx, 4, 1100)
    try:
        given.add_scene(range(4), sc, grid=True)
        same_result(ss.project_eval_resident(ctx, given, range(4), sc, masks, want_uv=True), want, "a supplied grid")
        same_result(ss.project_eval_resident(ctx, built, range(100, 104), sc, masks, want_uv=True), want, "a device-built grid")
    finally:
        given.close()


def test_pair_job_lists(ctx, pair):
    p, kfs, ps, want, store = pair
    N = p["N"]
    full = list(zip(ps.job_kf.tolist(), ps.job_K4.reshape(-1, 4), ps.job_src.reshape(-1, 12), ps.job_T.reshape(-1, 12), ps.job_pt0.tolist(), ps.job_n.tolist()))
    a, b = full
    cut = lambda j, p0, n: j[:4] + (p0, n)
    got = both_pair(ctx, store, [11, 12], ps, "both directions")
    assert got["n_hit"].min() > 300
    lists = {"an empty job first": [cut(a, 0, 0), b], "an empty job between": [a, cut(b, N, 0), cut(b, N + 5, 300)],
             "two jobs on one keyframe": [cut(a, 0, 400), cut(a, 400, N - 400), b], "overlapping ranges": [cut(a, 0, 700), cut(a, 300, 600), cut(b, N, 257), cut(b, N + 100, 257)],
             "no job": []}
    for n in (1, 63, 64, 65, 255, 256, 257):
        lists[f"{n} pairs"] = [cut(a, 40, n), cut(b, N + 7, n)]
    for name, jobs in lists.items():
        ps.set_jobs(jobs)
        try:
            both_pair(ctx, store, [11, 12], ps, name)
        finally:
            ps.set_jobs(full)
    # the keys in the other order: job_kf follows
    ps.set_jobs([(1 - j[0],) + j[1:] for j in full])
    try:
        same_result(ss.pair_eval_resident(ctx, store, [12, 11], ps, want_uv=True), want, "keys swapped")
    finally:
        ps.set_jobs(full)
    empty = ss.PairScene(kfs, 4.0, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, np.uint8), [cut(a, 0, 0)])
    assert both_pair(ctx, store, [11, 12], empty, "P = 0")["table"].size == 0
    none = ss.PairScene(kfs.subset([]), 4.0, ps.pos, ps.min_dist, ps.max_dist, ps.pt_desc, [])
    assert both_pair(ctx, store, [], none, "K = 0")["table"].size == 0


def test_planted_pairs(ctx):
    pl = pair_planted()
    ps = pl.scene()
    st = ks.KeyFrameStore(ctx, ps.kfs.K, 8)
    try:
        st.add_scene(range(ps.kfs.K), ps.kfs, grid=True)
        pl.check(both_pair(ctx, st, list(range(ps.kfs.K)), ps, "planted pairs"), "device")
    finally:
        st.close()


def test_a_key_that_is_not_live_is_refused_with_nothing_launched_and_the_next_call_is_correct(ctx, four, pair):
    sc, masks, want, store = four
    sub = sc.subset([1, 2], 300)
    table = np.full(600, 0xDEADBEEF, np.uint32); nv = np.full(2, -5, np.int32); nh = np.full(2, -5, np.int32)
    for keys in ([101, 999], [999, 101]):
        k, off, sk, sh, args = ss._resident_project(keys, sub, [masks[1], masks[1]], [0, 0], None)
        assert ss._dev().ccm_sim3_project_eval_resident(ctx.handle, store.raw, *args, ss._p(table), ss._p(nv), ss._p(nh), None) == -1      # CCM_E_ARG
        assert (table == 0xDEADBEEF).all() and (nv == -5).all()
    with pytest.raises(ss.CcmError):                        # a mask that is not as long as the key's features
        ss.project_eval_resident(ctx, store, [101, 102], sub, [masks[1], masks[2][:-1]])
    with pytest.raises(ss.CcmError):
        ss.project_eval_resident(ctx, store, [101, 102], sub, skip=(np.array([1, 2, 3], np.int32), np.zeros(4000, np.uint8)))
    both_proj(ctx, store, [101, 102], sub, [masks[1], masks[2]], "after the refusals")
    p, kfs, ps, pwant, pstore = pair
    t2 = np.full(ps.total, 0xDEADBEEF, np.uint32); nv = np.full(2, -5, np.int32); nh = np.full(2, -5, np.int32)
    keys = ks._keys([11, 999])
    assert ss._dev().ccm_sim3_pair_eval_resident(ctx.handle, pstore.raw, 2, ss._p(keys), *ps.tail(), ss._p(t2), ss._p(nv), ss._p(nh), None) == -1
    assert (t2 == 0xDEADBEEF).all() and (nv == -5).all()
    old = ps.job_T; ps.job_T = None
    try:
        with pytest.raises(ss.CcmError):
            ss.pair_eval_resident(ctx, pstore, [11, 12], ps)
    finally:
        ps.job_T = old
    same_result(ss.pair_eval_resident(ctx, pstore, [11, 12], ps, want_uv=True), pwant, "pair, after the refusals")


def test_the_projection_scene_and_its_mirror_on_the_device(ctx, frames):
    case = projection_case(frames)
    rlib = C.CDLL(trm.LIB) if HAVE_REF else None
    store = ks.KeyFrameStore(ctx, 2, 1100)
    try:
        for th in (10, 4):
            sc = projection_scene(frames, case, th)
            if th == 10:
                store.add_scene([70], sc, grid=True)
            m0 = (case["matched0"] >= 0).astype(np.uint8)
            got = both_proj(ctx, store, [70], sc, [m0], th)
            host_store = ks.KeyFrameStore(None, 1, 1100)
            host_store.add_scene([70], sc, grid=True)
            dev, cpu = ss.Sim3ProjectionSearch(store, 70, sc, m0), ss.Sim3ProjectionSearch(host_store, 70, sc, m0)
            try:
                assert np.array_equal(dev.table()["table"], got["table"][0])
                ra, rb = dev.resolve(case["matched0"], None, case["existing"]), cpu.resolve(case["matched0"], None, case["existing"])
                assert ra[0] == rb[0] > 600 and all(np.array_equal(x, y) for x, y in zip(ra[1:], rb[1:]))
                assert dev.n_reeval() == cpu.n_reeval() == expected_reeval(got["table"][0], None, ra[1]) > 0
                if rlib is not None:
                    n, ref_matched = ref_projection(rlib, case, th)[:2]
                    assert ra[0] == n and np.array_equal(ra[1], ref_matched)
            finally:
                dev.close(); cpu.close(); host_store.close()
    finally:
        store.close()


def test_the_pair_scene_and_its_mirror_on_the_device(ctx, pair):
    p, kfs, ps, want, store = pair
    s1, s2 = pair_sides(p)
    host_store = ks.KeyFrameStore(None, 2, 1100)
    host_store.add_scene([11, 12], kfs, grid=True)
    try:
        dev = ss.search_by_sim3(store, 11, 12, s1, s2, p["s12"], p["R12"], p["t12"], p["pre12"], p["sf"], p["th"])
        cpu = ss.search_by_sim3(host_store, 11, 12, s1, s2, p["s12"], p["R12"], p["t12"], p["pre12"], p["sf"], p["th"])
        assert dev["nFound"] == cpu["nFound"] > 300
        for k in ("matches12", "vnMatch1", "vnMatch2", "n_valid", "n_hit"):
            assert np.array_equal(dev[k], cpu[k]), k
        if HAVE_REF:
            n, out12 = ref_pair(C.CDLL(trm.LIB), p)[:2]
            assert dev["nFound"] == n and np.array_equal(dev["matches12"], out12)
    finally:
        host_store.close()


def test_two_threads_two_contexts_one_store(four, pair):
    """each thread makes 10 calls of one entry with a context of its own on the stores the other thread reads too; every answer equals the solo one"""
    from ccm_slam_amd._lib import Context
    sc, masks, want, store = four
    p, kfs, ps, pwant, pstore = pair
    errs = []

    def proj_thread():
        try:
            c = Context(0)
            try:
                for i in range(10):
                    same_result(ss.project_eval_resident(c, store, range(100, 104), sc, masks, want_uv=True), want, f"projection call {i}")
                    same_result(ss.pair_eval_resident(c, pstore, [11, 12], ps, want_uv=True), pwant, f"pair call {i} of the projection thread")
            finally:
                c.close()
        except BaseException as e:   # noqa: BLE001
            errs.append(e)

    def pair_thread():
        try:
            c = Context(0)
            try:
                for i in range(10):
                    same_result(ss.pair_eval_resident(c, pstore, [11, 12], ps, want_uv=True), pwant, f"pair call {i}")
                    same_result(ss.project_eval_resident(c, store, [103, 100], sc.subset([3, 0]), [masks[3], masks[0]], want_uv=True),
                                {k: (v[[3, 0]] if k != "uv" else v[[3, 0]]) for k, v in want.items()}, f"projection call {i} of the pair thread")
            finally:
                c.close()
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=proj_thread), threading.Thread(target=pair_thread)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
