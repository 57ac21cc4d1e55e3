"""CPU: ComputeSim3's SearchByBoW on keyframes of a HOST-ONLY keyframe store.  The host evaluator of ccm_bow_pair_eval_resident
(csrc/bow_search_math.h) against the per-query reduction of the Python replay; cslam::SearchByBoWBatch with ctx == nullptr against oracle.search_by_bow_kf_kf and,
where oracle/_ref is built, against the reference's own ORBmatcher.cpp; reevaluated() against the independent count; the refusals of set_featvec one by one."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import tests.test_ref_matcher as trm
from bow_search_cases import Kf, add_keyframe, expected_reeval, frame_case, fv_of, install, planted_cases, replay, same_words
from ccm_slam_amd import bow_search as bs, kfstore as ks, synth

HAVE_REF = os.path.exists(trm.LIB)
SETTINGS = ((0.75, 1), (0.7, 1), (0.9, 0))


@pytest.fixture(scope="module")
def frames():
    o = oracle.OrbOracle(1000)
    out = [o.extract(synth.gen_image(1000, t)) for t in (0, 1)]
    o.close()
    return out


@pytest.fixture(scope="module")
def cases(frames):
    """every case under its own pair of keys in one host-only store"""
    all_cases = planted_cases() + [frame_case(frames, 60), frame_case(frames, 6)]
    store = ks.KeyFrameStore(None, 2 * len(all_cases), 1100)
    for i, c in enumerate(all_cases):
        install(store, 2 * i, 2 * i + 1, c)
    yield store, all_cases
    store.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _oracle_args(c):
    k1, k2 = c.kf1, c.kf2
    return k1.fv, k2.fv, k1.live, k2.live, k1.desc, k1.angle, k2.desc, k2.angle


def test_host_evaluator_against_the_replays_reduction(cases):
    store, all_cases = cases
    for i, c in enumerate(all_cases):
        got = bs.pair_eval_host(store, [(2 * i, 2 * i + 1, c.kf1.live, c.kf2.live)])
        same_words(got, got["off"], 0, c, c.name)
    # all cases as one job list: every job's words and counters are what they are alone
    got = bs.pair_eval_host(store, [(2 * i, 2 * i + 1, c.kf1.live, c.kf2.live) for i, c in enumerate(all_cases)])
    for i, c in enumerate(all_cases):
        same_words(got, got["off"], i, c, (c.name, "in a list"))


def test_planted_properties(cases):
    store, all_cases = cases
    by = {c.name: (i, c) for i, c in enumerate(all_cases)}

    def words(name):
        i, c = by[name]
        return c, bs.unpack(bs.pair_eval_host(store, [(2 * i, 2 * i + 1, c.kf1.live, c.kf2.live)])["table"])
    c, u = words("all descriptors equal")
    firsts = {int(nd): int(c.kf2.fv[2][c.kf2.fv[1][b]]) for b, nd in enumerate(c.kf2.fv[0])}
    node1 = np.repeat(c.kf1.fv[0], np.diff(c.kf1.fv[1]))[np.argsort(c.kf1.fv[2])]
    assert (u["status"] == 2).all() and (u["d1"] == 0).all() and (u["d2"] == 0).all()
    assert [int(x) for x in u["idx"]] == [firsts[int(nd)] for nd in node1]
    c, u = words("ties across the pass boundary")
    p7 = c.kf2.fv[2][c.kf2.fv[1][0]:c.kf2.fv[1][1]]; p8 = c.kf2.fv[2][c.kf2.fv[1][1]:c.kf2.fv[1][2]]
    assert (u["d1"][0], u["idx"][0], u["d2"][0]) == (3, p7[63], 3)
    assert (u["d1"][1], u["idx"][1], u["d2"][1]) == (2, p8[64], 3)
    c, u = words("absent nodes, single candidate, all candidates masked, stopped words")
    node_of = -np.ones(c.kf1.n, int)
    node_of[c.kf1.fv[2]] = np.repeat(c.kf1.fv[0], np.diff(c.kf1.fv[1]))
    assert (u["status"][np.isin(node_of, (1, 25, 40, -1))] == 0).all()
    assert (u["status"][node_of == 35] == 1).all() and (u["d1"][node_of == 35] == 256).all() and (u["idx"][node_of == 35] == -1).all()
    assert (u["status"][node_of == 30] == 2).all() and (u["d2"][node_of == 30] == 256).all() and (u["d1"][node_of == 30] < 10).all()
    assert sorted(u["status"][node_of == 20]) == [0] + [2] * 6
    nm, m12, _ = replay(c, 0.75, 0)
    assert (m12[node_of == 30] >= 0).sum() == 1          # one candidate: the first query claims it, the others find nothing
    c, u = words("every query masked")
    assert not u["status"].any()


@pytest.mark.parametrize("nnratio,ori", SETTINGS)
def test_batch_against_the_oracle_and_the_replay(cases, nnratio, ori):
    store, all_cases = cases
    for i, c in enumerate(all_cases):
        exp_n, exp = oracle.search_by_bow_kf_kf(*_oracle_args(c), nnratio, ori)
        rep_n, rep, changed = replay(c, nnratio, ori)
        assert rep_n == exp_n and np.array_equal(rep, exp), c.name
        got = bs.search_by_bow_batch(store, 2 * i, [2 * i + 1], c.kf1.live, [c.kf2.live], nnratio, ori)
        assert got["nmatches"][0] == exp_n and np.array_equal(got["matches12"][0], exp), c.name
        assert got["reevaluated"] == expected_reeval(c, nnratio), c.name
        if c.name.startswith("frames"):
            # a comparison that finds no matches, or in which no claim ever matters, shows nothing
            assert exp_n > 100 and changed >= 1 and got["reevaluated"] >= 1, (c.name, exp_n, changed, got["reevaluated"])


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref not built")
@pytest.mark.parametrize("nnratio,ori", SETTINGS)
def test_batch_against_the_references_own_matcher(cases, nnratio, ori):
    store, all_cases = cases
    rlib = C.CDLL(trm.LIB)
    for i, c in enumerate(all_cases):
        k1, k2 = c.kf1, c.kf2
        ref = np.zeros(k1.n, np.int32)
        n = rlib.ref_search_by_bow_kf_kf(_p(k1.fv[0]), _p(k1.fv[1]), _p(k1.fv[2]), k1.fv[0].size, _p(k2.fv[0]), _p(k2.fv[1]), _p(k2.fv[2]), k2.fv[0].size, _p(k1.live),
                                         _p(k2.live), _p(k1.desc), _p(k1.angle), k1.n, _p(k2.desc), _p(k2.angle), k2.n, C.c_float(nnratio), ori, _p(ref))
        got = bs.search_by_bow_batch(store, 2 * i, [2 * i + 1], k1.live, [k2.live], nnratio, ori)
        assert got["nmatches"][0] == n and np.array_equal(got["matches12"][0], ref), c.name


def test_batch_of_three_candidates_and_no_candidate(cases, frames):
    """one current keyframe against three candidates (a frame, the frame again under another mask, itself): each is what the single call gives"""
    store, all_cases = cases
    i = len(all_cases) - 2
    c = all_cases[i]
    rng = np.random.default_rng(5)
    other = (rng.random(c.kf2.n) < 0.5).astype(np.uint8)
    got = bs.search_by_bow_batch(store, 2 * i, [2 * i + 1, 2 * i + 1, 2 * i], c.kf1.live, [c.kf2.live, other, c.kf1.live], 0.75, 1)
    singles = [bs.search_by_bow_batch(store, 2 * i, [k], c.kf1.live, [m], 0.75, 1) for k, m in ((2 * i + 1, c.kf2.live), (2 * i + 1, other), (2 * i, c.kf1.live))]
    for j, s in enumerate(singles):
        assert got["nmatches"][j] == s["nmatches"][0] and np.array_equal(got["matches12"][j], s["matches12"][0]), j
    assert got["reevaluated"] == sum(s["reevaluated"] for s in singles)
    # a keyframe against itself: every live feature's best candidate is itself at distance 0
    live = c.kf1.live > 0
    in_node = np.zeros(c.kf1.n, bool); in_node[c.kf1.fv[2]] = True
    u = bs.unpack(got["table"][2 * c.kf1.n:])
    assert (u["d1"][live & in_node] == 0).all()
    empty = bs.search_by_bow_batch(store, 2 * i, [], c.kf1.live, [], 0.75, 1)
    assert empty["nmatches"] == [] and empty["reevaluated"] == 0


def _snapshot(store, key, live_n):
    """what a refusal must leave alone: the key's vector as the evaluator reads it"""
    return bs.pair_eval_host(store, [(key, key, np.ones(live_n, np.uint8), np.ones(live_n, np.uint8))])


def test_set_featvec_refusals_leave_the_store_as_it_was():
    rng = np.random.default_rng(9)
    n = 12
    node_of = np.array([3, 3, 5, 5, 5, 9, 9, -1, 3, 9, 5, -1])
    kf = Kf(rng.integers(0, 256, (n, 32), dtype=np.uint8), np.zeros(n), fv_of(node_of), np.ones(n))
    store = ks.KeyFrameStore(None, 2, 64)
    add_keyframe(store, 7, kf)
    before = _snapshot(store, 7, n)
    assert before["n_query"][0] == 10
    node, off, idx = (x.copy() for x in kf.fv)

    def refused(nn, node, off, idx, key=7):
        with pytest.raises(ks.StoreError) as e:
            store.set_featvec(key, (nn, node, off, idx))
        assert e.value.code == ks.E_ARG
        after = _snapshot(store, 7, n)
        assert np.array_equal(after["table"], before["table"]) and after["n_dist"][0] == before["n_dist"][0]
    refused(3, node, off, idx, key=8)                                  # a key that is not live
    refused(-1, node, off, idx)
    refused(3, None, off, idx); refused(3, node, None, idx); refused(3, node, off, None)
    refused(3, np.array([3, 3, 9]), off, idx)                          # not strictly ascending
    refused(3, np.array([5, 3, 9]), off, idx)
    refused(3, np.array([-1, 5, 9]), off, idx)                         # negative
    refused(3, node, off + 1, idx)                                     # off[0] != 0
    refused(3, node, np.array([0, 3, 3, 10]), idx)                     # an empty node
    refused(3, node, np.array([0, 3, 2, 10]), idx)
    bad = idx.copy(); bad[4] = n
    refused(3, node, off, bad)                                         # outside [0, n)
    bad = idx.copy(); bad[0] = -1
    refused(3, node, off, bad)
    bad = idx.copy(); bad[[0, 1]] = bad[[1, 0]]
    refused(3, node, off, bad)                                         # not ascending inside a node
    bad = idx.copy(); bad[4] = bad[0]
    refused(3, node, off, bad)                                         # a feature listed twice (in two nodes)
    bad = idx.copy(); bad[1] = bad[0]
    refused(3, node, off, bad)                                         # a feature listed twice (in one node)
    # legal: off[nn] < n (the stopped words), nn == 0, and a second call replaces the first
    store.set_featvec(7, (0, None, None, None))
    assert _snapshot(store, 7, n)["n_query"][0] == 0
    store.set_featvec(7, fv_of(np.where(node_of == 9, -1, node_of)))
    assert _snapshot(store, 7, n)["n_query"][0] == 7
    store.set_featvec(7, kf.fv)
    assert np.array_equal(_snapshot(store, 7, n)["table"], before["table"])
    store.close()


def test_host_only_store_lifetime_and_evaluator_refusals():
    rng = np.random.default_rng(10)
    mk = lambda n, seed: Kf(np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8), np.zeros(n), fv_of(rng.integers(0, 4, n)), np.ones(n))
    a, b = mk(20, 1), mk(30, 2)
    store = ks.KeyFrameStore(None, 2, 64)
    add_keyframe(store, 1, a); add_keyframe(store, 2, b, featvec=False)
    ones = lambda n: np.ones(n, np.uint8)
    with pytest.raises(Exception):
        bs.pair_eval_host(store, [(1, 2, ones(20), ones(30))])         # key 2 has no feature vector
    with pytest.raises(Exception):
        bs.pair_eval_host(store, [(1, 3, ones(20), ones(30))])         # key 3 is not live
    store.set_featvec(2, b.fv)
    ok = bs.pair_eval_host(store, [(1, 2, ones(20), ones(30))])
    assert ok["n_query"][0] > 0
    with pytest.raises(Exception):
        bs.pair_eval_host(store, [(1, 2, ones(19), ones(30))])         # a mask that is not as long as the keyframe
    # erase, and a new tenant under the same key without a vector: refused, no stale vector
    store.erase(2)
    add_keyframe(store, 2, b, featvec=False)
    with pytest.raises(Exception):
        bs.pair_eval_host(store, [(1, 2, ones(20), ones(30))])
    store.clear()
    add_keyframe(store, 1, a, featvec=False)
    with pytest.raises(Exception):
        bs.pair_eval_host(store, [(1, 1, ones(20), ones(20))])
    store.close()
