"""CPU: the host evaluator of ccm_mappoint_refresh_resident (csrc/mappoint_math.h through libccm_host.so) on a host-only store, every comparison
exact (integers as integers, floats as bit patterns, a NaN matches a NaN) and on every point of every case: against the numpy replay of tests/mappoint_cases.py,
against oracle.distinctive_descriptors and oracle.update_normal_and_depth, against the reference's own MapPoint.cpp where oracle/_ref is built, the host mirror
cslam::MapPointRefresh without a context, and every refusal with the outputs untouched."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import oracle
import tests.test_ref_matcher as trm
from mappoint_cases import KEYS, MAX_FEAT, NLEVELS, SF, Cases, call, flatten, install, planted, replay, replay_normal_depth, same, same_f32, todays_inputs
from ccm_slam_amd import kfstore as ks, mappoint as mp

HAVE_REF = os.path.exists(trm.LIB) or os.path.isdir("/root/reference/cslam")


@pytest.fixture(scope="module")
def cases():
    cs = planted()
    store = ks.KeyFrameStore(None, 8, MAX_FEAT)
    install(store, cs)
    yield store, cs
    store.close()


@pytest.fixture(scope="module")
def everything(cases):
    """all cases in one call: the arrays, the host evaluator's answer and the replay's, computed once"""
    store, cs = cases
    f = flatten(cs, cs.all_points())
    return f, call(mp.refresh_host, (store,), f), replay(cs, cs.all_points())


def test_host_evaluator_against_the_replay(cases, everything):
    store, cs = cases
    for c in cs.cases:
        same(call(mp.refresh_host, (store,), flatten(cs, c.points)), replay(cs, c.points), c.name)
    f, got, want = everything
    same(got, want, "all cases in one call")
    # what the cases are there for
    st = lambda name: [int(x) for x in replay(cs, cs.by_name(name).points)["status"]]
    assert st("an empty list") == [0, 0] and st("ref_kf = -1") == [mp.DESC] * 2 and st("a reference octave beyond the tables") == [mp.DESC | mp.OCTAVE_BEYOND] * 3
    assert st("the reference octave nlevels - 1") == [mp.DESC | mp.NORMAL_DEPTH] * 2
    two = replay(cs, cs.by_name("N=2 of unrelated descriptors: the rank is 0, index 0 wins").points)
    assert two["best_obs"].tolist() == [0, 0]
    assert replay(cs, cs.by_name("equal least medians, the earlier wins").points)["best_obs"].tolist() == [1, 0]
    assert replay(cs, cs.by_name("the least median at the last index").points)["best_obs"].tolist() == [4]
    assert replay(cs, cs.by_name("identical descriptors").points)["best_obs"].tolist() == [0]
    assert replay(cs, cs.by_name("complementary descriptors: a distance of 256").points)["best_obs"].tolist() == [0, 1, 1]
    at = replay(cs, cs.by_name("an observer exactly at the point").points)
    assert np.isnan(at["normal"]).all() and at["max_dist"][1] == 0 and at["min_dist"][1] == 0 and at["max_dist"][0] > 0
    empty = cs.by_name("an empty list").points
    kept = call(mp.refresh_host, (store,), flatten(cs, empty))
    assert same_f32(kept["normal"], np.stack([p.seed[:3] for p in empty])) and kept["best_obs"].tolist() == [-1, -1] and kept["min_dist"][0] == empty[0].seed[3]


def test_the_order_of_the_list_matters(cases):
    """the planted lists are ones whose f32 sum changes its bits under some permutation: a kernel that adds in another order cannot pass"""
    _, cs = cases
    p = cs.by_name("the sum runs in list order").points[0]
    centres = [cs.centres[k] for k, _ in p.obs]
    base = replay_normal_depth(p.pos, centres, centres[0], 0, SF)[0]
    assert any(not same_f32(replay_normal_depth(p.pos, [centres[i] for i in perm], centres[0], 0, SF)[0], base) for perm in itertools.permutations(range(len(centres))))
    q = cs.by_name("the sum runs in list order").points[1]
    centres = [cs.centres[k] for k, _ in q.obs]
    assert not same_f32(replay_normal_depth(q.pos, centres[::-1], centres[0], 0, SF)[0], replay_normal_depth(q.pos, centres, centres[0], 0, SF)[0])


def test_host_evaluator_against_the_oracle(cases, everything):
    store, cs = cases
    f, got, _ = everything
    t = todays_inputs(cs, f)
    assert np.array_equal(got["best_obs"], oracle.distinctive_descriptors(t["desc"], f["obs_off"]))
    nrm, dmin, dmax = oracle.update_normal_and_depth(f["pos"], f["obs_off"], f["obs_kf"], f["kf_center"], t["ref_kf"], t["ref_level"], SF, f["normal"], f["min_dist"], f["max_dist"])
    ran = (got["status"] & mp.NORMAL_DEPTH) != 0
    assert np.array_equal(ran, t["ok"] & (np.diff(f["obs_off"]) > 0)) and ran.sum() > 30
    assert same_f32(got["normal"][ran], nrm.reshape(-1, 3)[ran]) and same_f32(got["min_dist"][ran], dmin[ran]) and same_f32(got["max_dist"][ran], dmax[ran])
    # a point whose part did not run keeps its values
    assert same_f32(got["normal"][~ran], f["normal"][~ran]) and same_f32(got["min_dist"][~ran], f["min_dist"][~ran]) and same_f32(got["max_dist"][~ran], f["max_dist"][~ran])


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref not built")
def test_host_evaluator_against_the_references_mappoint(cases, everything):
    """MapPoint::ComputeDistinctiveDescriptors, the reference's own lines (oracle/_ref), on the gathered rows of every point"""
    _, cs = cases
    f, got, _ = everything
    if not os.path.exists(trm.LIB):
        trm.ref.build()
    rlib = C.CDLL(trm.LIB)
    t = todays_inputs(cs, f)
    desc = np.ascontiguousarray(t["desc"]); off = np.ascontiguousarray(f["obs_off"])
    ref = np.zeros(off.size - 1, np.int32)
    rlib.ref_distinctive_descriptors(trm._p(desc), trm._p(off), off.size - 1, trm._p(ref))
    # the driver reports the FIRST row that equals the descriptor the point took, so rows that are equal byte for byte are one answer: every point ends up with the
    # same 32 bytes, and with the same index wherever the winner's row occurs once in its list
    n = np.diff(off)
    assert np.array_equal(ref[n == 0], got["best_obs"][n == 0]) and (ref[n == 0] == -1).all()
    once = 0
    for p in np.flatnonzero(n > 0):
        rows = desc[off[p]:off[p + 1]]
        assert np.array_equal(rows[ref[p]], got["best_desc"][p]), p
        if (rows == rows[ref[p]]).all(1).sum() == 1:
            assert ref[p] == got["best_obs"][p], p
            once += 1
    assert once > 40


def test_mirror_without_a_context(cases, everything):
    store, cs = cases
    f, want, _ = everything
    with mp.Refresh(store, *[f[k] for k in ("keys", "kf_center", "obs_off", "obs_kf", "obs_feat", "pos", "ref_kf", "ref_feat", "scale_factors", "normal", "min_dist",
                                            "max_dist")], host=True) as m:
        got = m.result()
    same(got, want, "the host mirror")
    assert np.array_equal(got["has_desc"] != 0, want["best_obs"] >= 0)
    with pytest.raises(mp.CcmError):
        mp.Refresh(store, [4242], f["kf_center"][:1], [0, 1], [0], [0], f["pos"][:1], [0], [0], SF, f["normal"][:1], f["min_dist"][:1], f["max_dist"][:1], host=True)


def refusals(cs: Cases):
    """(why, the raw arguments K, keys, kf_center, P, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, nlevels, sf, and which outputs are null) for a call of two
    points that is right, with one thing wrong each"""
    n0, n1 = cs.kfs[0]["oct"].size, cs.kfs[1]["oct"].size
    good = dict(K=2, keys=KEYS[:2], kf_center=cs.centres[:2], P=2, obs_off=[0, 2, 3], obs_kf=[0, 1, 1], obs_feat=[0, 1, n1 - 1], pos=np.ones((2, 3), np.float32), ref_kf=[1, -1],
                ref_feat=[n1 - 1, 0], nlevels=NLEVELS, scale_factors=SF, null=())
    out = [("nothing", good)]
    for why, change in [("a key that is not live", dict(keys=[100, 4242])), ("obs_off not starting at 0", dict(obs_off=[1, 2, 3])), ("obs_off decreasing", dict(obs_off=[0, 2, 1])),
                        ("obs_kf = K", dict(obs_kf=[0, 2, 1])), ("obs_kf negative", dict(obs_kf=[0, -1, 1])), ("obs_feat = n", dict(obs_feat=[n0, 1, 0])),
                        ("obs_feat negative", dict(obs_feat=[0, -1, 0])), ("ref_feat = n", dict(ref_feat=[n1, 0])), ("ref_feat negative", dict(ref_feat=[-1, 0])),
                        ("ref_kf = K", dict(ref_kf=[2, -1])), ("ref_kf = -2", dict(ref_kf=[1, -2])), ("nlevels 0", dict(nlevels=0)), ("nlevels 257", dict(nlevels=257)),
                        ("P negative", dict(P=-1)), ("K negative", dict(K=-1)),
                        ("more than 256 observations", dict(P=1, obs_off=[0, 257], obs_kf=[0] * 257, obs_feat=[0] * 257, ref_kf=[0], ref_feat=[0])),
                        ("null keys", dict(keys=None)), ("null obs_off", dict(obs_off=None)), ("null obs_kf", dict(obs_kf=None)), ("null obs_feat", dict(obs_feat=None)),
                        ("null ref_kf", dict(ref_kf=None)), ("null ref_feat", dict(ref_feat=None)), ("null scale_factors", dict(scale_factors=None)),
                        ("null pos while a point has a reference", dict(pos=None)), ("null kf_center while a point has a reference", dict(kf_center=None)),
                        ("null best_obs", dict(null=("best_obs",))), ("null normal", dict(null=("normal",))), ("null min_dist", dict(null=("min_dist",))),
                        ("null max_dist", dict(null=("max_dist",))), ("null status", dict(null=("status",)))]:
        out.append((why, {**good, **change}))
    return out


def raw_call(ctx, store, a: dict):
    """the return code and the outputs, which start as marks"""
    P = 2
    out = dict(best_obs=np.full(P, -77, np.int32), best_desc=np.full((P, 32), 0xA5, np.uint8), normal=np.full(3 * P, -5.5, np.float32), min_dist=np.full(P, -6.5, np.float32),
               max_dist=np.full(P, -7.5, np.float32), status=np.full(P, 0x5A, np.uint8))
    given = {k: (None if k in a["null"] else v) for k, v in out.items()}
    rc = mp.refresh_raw(ctx, store, a["K"], a["keys"], a["kf_center"], a["P"], a["obs_off"], a["obs_kf"], a["obs_feat"], a["pos"], a["ref_kf"], a["ref_feat"], a["nlevels"],
                        a["scale_factors"], given)
    return rc, out


def untouched(out: dict) -> bool:
    return bool((out["best_obs"] == -77).all() and (out["best_desc"] == 0xA5).all() and (out["normal"] == -5.5).all() and (out["min_dist"] == -6.5).all() and
                (out["max_dist"] == -7.5).all() and (out["status"] == 0x5A).all())


def test_refusals_leave_the_outputs_untouched(cases):
    store, cs = cases
    for why, a in refusals(cs):
        rc, out = raw_call(None, store, a)
        if why == "nothing":
            assert rc == 0 and out["best_obs"].tolist() == [0, 0] and out["status"].tolist() == [mp.DESC | mp.NORMAL_DEPTH, mp.DESC], why
        else:
            assert rc == -1 and untouched(out), why
    rc, out = raw_call(None, None, refusals(cs)[0][1])
    assert rc == -1 and untouched(out)
    # legal: no point; no key and no observation; one key listed twice; pos and kf_center null when no point has a reference
    good = refusals(cs)[0][1]
    assert raw_call(None, store, {**good, "P": 0, "obs_off": None, "null": ("best_obs", "normal", "min_dist", "max_dist", "status")})[0] == 0
    rc, out = raw_call(None, store, {**good, "K": 0, "keys": None, "kf_center": None, "obs_off": [0, 0, 0], "obs_kf": None, "obs_feat": None, "ref_kf": [-1, -1], "pos": None})
    assert rc == 0 and out["best_obs"].tolist() == [-1, -1] and out["status"].tolist() == [0, 0] and (out["normal"] == -5.5).all() and (out["best_desc"] == 0xA5).all()
    rc, out = raw_call(None, store, {**good, "keys": [101, 101], "ref_kf": [-1, -1], "pos": None, "kf_center": None})
    assert rc == 0 and out["status"].tolist() == [mp.DESC, mp.DESC] and (out["normal"] == -5.5).all()
