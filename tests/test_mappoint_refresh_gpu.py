"""GPU: ccm_mappoint_refresh_resident against the host evaluator, exactly (integers as integers, floats as bit patterns, a NaN matches a NaN) on every
point: every planted case alone and all of them in one call, no point, with and without the winners' descriptors, today's route (ccm_distinctive_descriptors and
ccm_update_normal_and_depth through their wrappers) on the same data, the refusals and the call after each, a slot reused after an erase, cslam::MapPointRefresh on
the device against the host mirror, and two threads with their own contexts on one store."""
import threading

import numpy as np
import pytest

from mappoint_cases import KEYS, MAX_FEAT, REC, SF, call, flatten, install, planted, replay, same, same_f32, todays_inputs
from test_mappoint_refresh_cpu import raw_call, refusals, untouched
from ccm_slam_amd import frame, kfstore as ks, mappoint as mp, matcher

pytestmark = pytest.mark.gpu
MIRROR_ARGS = ("keys", "kf_center", "obs_off", "obs_kf", "obs_feat", "pos", "ref_kf", "ref_feat", "scale_factors", "normal", "min_dist", "max_dist")


@pytest.fixture(scope="module")
def cases(ctx):
    cs = planted()
    store = ks.KeyFrameStore(ctx, 9, MAX_FEAT)   # one slot more than the cases need: the reuse test takes it
    install(store, cs)
    yield store, cs
    store.close()


@pytest.fixture(scope="module")
def everything(cases):
    store, cs = cases
    f = flatten(cs, cs.all_points())
    return f, call(mp.refresh_host, (store,), f)


def test_every_case_alone_and_all_in_one_call(ctx, cases, everything):
    store, cs = cases
    for c in cs.cases:
        f = flatten(cs, c.points)
        want = call(mp.refresh_host, (store,), f)
        same(call(mp.refresh_resident, (ctx, store), f), want, c.name)
        same(want, replay(cs, c.points), (c.name, "the host evaluator against the replay"))
    f, want = everything
    same(call(mp.refresh_resident, (ctx, store), f), want, "all cases in one call")
    # the same points in reverse: other neighbours in a wave, other workgroups
    pts = cs.all_points()[::-1]
    f = flatten(cs, pts)
    same(call(mp.refresh_resident, (ctx, store), f), call(mp.refresh_host, (store,), f), "all cases in reverse")


def test_no_point_and_the_descriptors_optional(ctx, cases, everything):
    store, cs = cases
    got = call(mp.refresh_resident, (ctx, store), flatten(cs, []))
    assert got["best_obs"].size == 0 and got["status"].size == 0
    f, want = everything
    got = call(mp.refresh_resident, (ctx, store), f, want_desc=False)
    assert got["best_desc"] is None
    same(got, want, "without best_desc", desc=False)
    # an empty list leaves its row of best_desc as the caller had it
    a = refusals(cs)[0][1]
    rc, out = raw_call(ctx, store, {**a, "obs_off": [0, 2, 2]})
    assert rc == 0 and out["best_obs"].tolist() == [0, -1] and (out["best_desc"][1] == 0xA5).all() and not (out["best_desc"][0] == 0xA5).all()


def test_agrees_with_todays_route(ctx, cases, everything):
    store, cs = cases
    f, want = everything
    got = call(mp.refresh_resident, (ctx, store), f)
    t = todays_inputs(cs, f)
    assert np.array_equal(got["best_obs"], matcher.distinctive_descriptors(ctx, t["desc"], f["obs_off"]))
    nrm, dmin, dmax = frame.update_normal_and_depth(ctx, f["pos"], f["obs_off"], f["obs_kf"], f["kf_center"], t["ref_kf"], t["ref_level"], SF, f["normal"], f["min_dist"],
                                                    f["max_dist"])
    ran = (got["status"] & mp.NORMAL_DEPTH) != 0
    assert ran.sum() > 30
    assert same_f32(got["normal"][ran], nrm[ran]) and same_f32(got["min_dist"][ran], dmin[ran]) and same_f32(got["max_dist"][ran], dmax[ran])


def test_refusals_launch_nothing_and_the_next_call_is_right(ctx, cases):
    store, cs = cases
    probe = flatten(cs, cs.by_name("N=9").points + cs.by_name("N=65").points)
    want = call(mp.refresh_host, (store,), probe)
    for why, a in refusals(cs):
        rc, out = raw_call(ctx, store, a)
        if why == "nothing":
            assert rc == 0 and out["best_obs"].tolist() == [0, 0] and out["status"].tolist() == [mp.DESC | mp.NORMAL_DEPTH, mp.DESC], why
            continue
        assert rc == -1 and untouched(out), why
        same(call(mp.refresh_resident, (ctx, store), probe), want, ("the call after", why))
    rc, out = raw_call(ctx, None, refusals(cs)[0][1])
    assert rc == -1 and untouched(out)
    good = refusals(cs)[0][1]
    rc, out = raw_call(ctx, store, {**good, "K": 0, "keys": None, "kf_center": None, "obs_off": [0, 0, 0], "obs_kf": None, "obs_feat": None, "ref_kf": [-1, -1], "pos": None})
    assert rc == 0 and out["best_obs"].tolist() == [-1, -1] and out["status"].tolist() == [0, 0] and (out["normal"] == -5.5).all() and (out["best_desc"] == 0xA5).all()
    rc, out = raw_call(ctx, store, {**good, "keys": [101, 101], "ref_kf": [-1, -1], "pos": None, "kf_center": None})
    assert rc == 0 and out["status"].tolist() == [mp.DESC, mp.DESC] and (out["normal"] == -5.5).all()


def test_a_slot_reused_after_erase(ctx, cases):
    """key 500 takes the free slot, is erased, and key 501 moves into the slot with other descriptors and octaves: the call on 501 reads the new tenant's rows"""
    store, cs = cases
    rng = np.random.default_rng(4)
    n = 40
    lists = dict(kf_center=cs.centres[:2], obs_off=[0, 5, 25], obs_kf=[1] * 5 + [1, 0] * 10, obs_feat=list(range(5)) + list(range(20)), pos=np.ones((2, 3), np.float32),
                 ref_kf=[1, 1], ref_feat=[7, 8], scale_factors=SF)
    answers = []
    for key in (500, 501):
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8); octv = rng.integers(0, 8, n).astype(np.uint8)
        store.add([key], REC, [0, n], rng.uniform(20, 400, (n, 2)).astype(np.float32), octv, desc)
        keys = [100, key]
        want = mp.refresh_host(store, keys, **lists)
        got = mp.refresh_resident(ctx, store, keys, **lists)
        same(got, want, ("key", key))
        assert np.array_equal(got["best_desc"][0], desc[got["best_obs"][0]])
        answers.append(got)
        store.erase(key)
    assert not np.array_equal(answers[0]["best_desc"], answers[1]["best_desc"])
    out = dict(best_obs=np.zeros(2, np.int32), best_desc=None, normal=np.zeros(6, np.float32), min_dist=np.zeros(2, np.float32), max_dist=np.zeros(2, np.float32),
               status=np.zeros(2, np.uint8))
    assert mp.refresh_raw(ctx, store, 2, [100, 501], lists["kf_center"], 2, lists["obs_off"], lists["obs_kf"], lists["obs_feat"], lists["pos"], lists["ref_kf"],
                          lists["ref_feat"], SF.size, SF, out) == -1          # erased: not live


def test_mirror_on_the_device_against_the_host_mirror(cases, everything):
    store, cs = cases
    f, want = everything
    with mp.Refresh(store, *[f[k] for k in MIRROR_ARGS]) as m:
        got = m.result()
    with mp.Refresh(store, *[f[k] for k in MIRROR_ARGS], host=True) as m:
        host = m.result()
    same(got, host, "the device mirror against the host mirror")
    same(got, want, "the device mirror against the host evaluator")
    assert np.array_equal(got["has_desc"], host["has_desc"])


def test_two_threads_with_two_contexts_on_one_store(cases, everything):
    store, cs = cases
    f, want = everything
    results, errors = [None, None], []

    def work(t):
        try:
            for _ in range(3):
                with mp.Refresh(store, *[f[k] for k in MIRROR_ARGS]) as m:
                    results[t] = m.result()
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for r in results:
        same(r, want, "a thread's mirror")
