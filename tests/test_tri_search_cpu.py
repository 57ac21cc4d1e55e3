"""CPU: CreateNewMapPoints' SearchForTriangulation on keyframes of a HOST-ONLY keyframe store.  The host evaluator of ccm_tri_search_eval_resident
(csrc/tri_search_math.h) against the Python replay's words and counters; the planted properties by name; cslam::SearchForTriangulationBatch with ctx == nullptr
against oracle.search_for_triangulation, the replay and, where oracle/_ref is built, the reference's own ORBmatcher.cpp; a 6-neighbour sequence with map points
created between the calls; the re-evaluation rule against an independent count; every refusal of the evaluator."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import tests.test_ref_matcher as trm
from tri_search_cases import (K4, S2, SF, Case, Kf, add_keyframe, frame_case, fv_of, install, install_sequence, oracle_call, planted_cases, replay, run_sequence,
                              same_words, sequence_cases)
from ccm_slam_amd import kfstore as ks, synth, tri_search as ts

HAVE_REF = os.path.exists(trm.LIB)
MATCH_FLOOR = 40


@pytest.fixture(scope="module")
def frames():
    o = oracle.OrbOracle(1000)
    out = [o.extract(synth.gen_image(1000, t)) for t in (0, 1)]
    o.close()
    return out


@pytest.fixture(scope="module")
def cases(frames):
    """every case under its own pair of keys in one host-only store"""
    all_cases = planted_cases() + [frame_case(frames)]
    store = ks.KeyFrameStore(None, 2 * len(all_cases), 1100)
    for i, c in enumerate(all_cases):
        install(store, 2 * i, 2 * i + 1, c)
    yield store, all_cases
    store.close()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_host_evaluator_against_the_replay(cases):
    store, all_cases = cases
    for i, c in enumerate(all_cases):
        got = ts.pair_eval_host(store, [c.job(2 * i, 2 * i + 1)], SF, S2)
        same_words(got, got["off"], 0, c, c.name)
    # all cases as one job list: every job's words and counters are what they are alone
    got = ts.pair_eval_host(store, [c.job(2 * i, 2 * i + 1) for i, c in enumerate(all_cases)], SF, S2)
    for i, c in enumerate(all_cases):
        same_words(got, got["off"], i, c, (c.name, "in a list"))


def test_planted_properties(cases):
    store, all_cases = cases
    by = {c.name: (i, c) for i, c in enumerate(all_cases)}

    def words(name):
        i, c = by[name]
        node_of = -np.ones(c.kf1.n, int)
        node_of[c.kf1.fv[2]] = np.repeat(c.kf1.fv[0], np.diff(c.kf1.fv[1]))
        seg2 = {int(nd): c.kf2.fv[2][c.kf2.fv[1][b]:c.kf2.fv[1][b + 1]] for b, nd in enumerate(c.kf2.fv[0])}
        return c, ts.unpack(ts.pair_eval_host(store, [c.job(2 * i, 2 * i + 1)], SF, S2)["table"]), node_of, seg2

    def only(u, node_of, nd):
        (i,) = np.flatnonzero(node_of == nd)
        return int(u["status"][i]), int(u["idx"][i]), int(u["dist"][i])
    c, u, node_of, seg2 = words("ties")
    assert only(u, node_of, 7) == (2, seg2[7][64], 3)        # equal distances at positions 63 and 64: the later one
    assert only(u, node_of, 8) == (2, seg2[8][63], 2)        # the nearer one at 63 stays
    assert only(u, node_of, 9) == (2, seg2[9][11], 7)        # equal distances inside one pass: the later one
    c, u, node_of, seg2 = words("thresholds and gates")
    assert only(u, node_of, 31) == (2, seg2[31][2], 50)      # a candidate at TH_LOW is accepted
    assert only(u, node_of, 32) == (1, -1, 50)               # one at 51 is not
    assert only(u, node_of, 33) == (2, seg2[33][4], 20)      # the nearest fails the line gate, the farther one passes
    assert only(u, node_of, 34) == (2, seg2[34][3], 25)      # the nearest is inside the epipole's radius
    q35 = np.flatnonzero(node_of == 35)
    assert (u["status"][q35] == 2).all() and (u["idx"][q35] == seg2[35][3]).all() and sorted(u["dist"][q35]) == [6, 9]   # one idx2, kept by both
    for o in (0, 2):
        c, u, node_of, seg2 = words(f"dsqr one ulp below the threshold, octave {o}")
        assert (u["status"] == 2).all() and sorted(u["dist"]) == [2, 3, 4]
        c, u, node_of, seg2 = words(f"dsqr one ulp above the threshold, octave {o}")
        assert (u["status"] == 1).all()
    for name in ("den == 0", "NaN in F12"):
        c, u, node_of, seg2 = words(name)
        assert (u["status"] == 1).all() and (u["idx"] == -1).all() and (u["dist"] == 50).all()
    c, u, node_of, seg2 = words("the den / NaN keyframes on plain rows")
    assert (u["status"] == 2).all() and (u["dist"] == 3).all()
    c, u, node_of, seg2 = words("every candidate with a map point, every query with a map point")
    assert (u["status"][node_of == 3] == 1).all() and (u["status"][node_of == 5] == 0).all()
    i, c = by["every candidate with a map point, every query with a map point"]
    assert ts.pair_eval_host(store, [c.job(2 * i, 2 * i + 1)], SF, S2)["n_dist"][0] == 0
    c, u, node_of, seg2 = words("absent nodes, stopped words")
    assert (u["status"][np.isin(node_of, (1, 25, 40, -1))] == 0).all() and (u["status"][(node_of == 20) & (c.kf1.has == 0)] >= 1).all()
    c, u, node_of, seg2 = words("query nodes of 65 and 130")
    assert (u["status"][c.kf1.has == 0] >= 1).all() and (u["status"] == 2).sum() > 20


@pytest.mark.parametrize("ori", (1, 0))
def test_batch_against_the_oracle_and_the_replay(cases, ori):
    """The frame scene: the oracle finds 95 matches with the orientation filter and 96 without it on this scene; the floor of 40 lies well below both."""
    store, all_cases = cases
    for i, c in enumerate(all_cases):
        exp_n, exp = oracle_call(c, ori)
        rep_n, rep, _, _ = replay(c, ori)
        assert rep_n == exp_n and np.array_equal(rep, exp), c.name
        got = ts.search_for_triangulation_batch(store, 2 * i, [2 * i + 1], c.kf1.has, [c.kf2.has], [(c.F12, c.ex, c.ey)], S2, SF, ori)
        assert got["nmatches"][0] == exp_n and np.array_equal(got["matches12"][0], exp), c.name
        assert got["reevaluated"] == 0
        if c.name.startswith("frames"):
            print("frame scene matches:", exp_n)
            assert exp_n > MATCH_FLOOR, (c.name, exp_n)   # a comparison that finds no matches shows nothing


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref not built")
@pytest.mark.parametrize("ori", (1, 0))
def test_batch_against_the_references_own_matcher(cases, ori):
    store, all_cases = cases
    rlib = C.CDLL(trm.LIB)
    T1 = np.eye(4, dtype=np.float32)
    for i, c in enumerate(all_cases):
        k1, k2 = c.kf1, c.kf2
        T2 = np.eye(4, dtype=np.float32); T2[:3, 3] = c.t2
        ref = np.zeros(k1.n, np.int32); ex = C.c_float(0); ey = C.c_float(0)
        n = rlib.ref_search_for_triangulation(_p(k1.fv[0]), _p(k1.fv[1]), _p(k1.fv[2]), k1.fv[0].size, _p(k2.fv[0]), _p(k2.fv[1]), _p(k2.fv[2]), k2.fv[0].size, _p(k1.has),
                                              _p(k2.has), _p(k1.desc), _p(k1.x), _p(k1.y), _p(k1.angle), k1.n, _p(k2.desc), _p(k2.x), _p(k2.y), _p(k2.octave),
                                              _p(k2.angle), k2.n, _p(c.F12), _p(T1), _p(T2), _p(K4), _p(S2), _p(SF), ori, _p(ref), C.byref(ex), C.byref(ey))
        assert (np.float32(ex.value), np.float32(ey.value)) == (c.ex, c.ey), c.name     # the case's epipole is the reference's own
        got = ts.search_for_triangulation_batch(store, 2 * i, [2 * i + 1], k1.has, [k2.has], [(c.F12, c.ex, c.ey)], S2, SF, ori)
        assert got["nmatches"][0] == n and np.array_equal(got["matches12"][0], ref), c.name


@pytest.fixture(scope="module")
def sequence(frames):
    return sequence_cases(frames)


def test_six_neighbour_sequence_with_points_created_between_the_calls(sequence):
    seq, has1 = sequence
    store = ks.KeyFrameStore(None, 8, 1100)
    install_sequence(store, seq)
    total, _ = run_sequence(store, seq, has1, host=True)
    print("sequence matches:", total)
    assert total > 100      # the oracle's own total on these six neighbours is 223
    store.close()


def _expected_reeval(case: Case, has1_now, has2_now):
    """independently of the mirror: the queries that have a word (no map point at the build, in a common node), are still queries now, and whose word's bestIdx2 has
    a map point now or whose node's segment of keyframe 2 holds a feature that lost one"""
    k1, k2 = case.kf1, case.kf2
    _, _, words, _ = replay(case, 0)
    pos2 = {int(nd): b for b, nd in enumerate(k2.fv[0])}
    count = 0
    for a, nd in enumerate(k1.fv[0]):
        if int(nd) not in pos2:
            continue
        seg = k2.fv[2][k2.fv[1][pos2[int(nd)]]:k2.fv[1][pos2[int(nd)] + 1]]
        lost = bool(((k2.has[seg] != 0) & (has2_now[seg] == 0)).any())
        for idx1 in k1.fv[2][k1.fv[1][a]:k1.fv[1][a + 1]]:
            if k1.has[idx1] or has1_now[idx1]:
                continue
            count += lost or (words[idx1, 1] >= 0 and has2_now[words[idx1, 1]] != 0)
    return count


def test_winner_gained_a_point_and_a_node_lost_one(cases):
    store, all_cases = cases
    i = len(all_cases) - 1
    c = all_cases[i]
    _, m0, _, _ = replay(c, 0)
    winners = m0[m0 >= 0]
    assert winners.size > MATCH_FLOOR
    rng = np.random.default_rng(4)
    # (a) a third of the winners gain a map point, and so do some features that are nobody's winner
    gained = c.kf2.has.copy()
    gained[winners[::3]] = 1
    gained[rng.choice(np.flatnonzero(gained == 0), 40, replace=False)] = 1
    # (b) features of keyframe 2 lose their map point (new candidates), and a feature of keyframe 1 that had one at the build loses it (it has no word)
    lost = c.kf2.has.copy()
    lost[np.flatnonzero(c.kf2.has)[::4]] = 0
    has1_lost = c.kf1.has.copy()
    has1_lost[np.flatnonzero(c.kf1.has)[::5]] = 0
    both = gained.copy(); both[lost == 0] = 0
    for ori in (0, 1):
        with ts.Batch(store, 2 * i, [2 * i + 1], c.kf1.has, [c.kf2.has], [(c.F12, c.ex, c.ey)], S2, SF, ori) as b:
            seen = 0
            for has1_now, has2_now in ((c.kf1.has, gained), (c.kf1.has, lost), (has1_lost, lost), (has1_lost, both), (c.kf1.has, c.kf2.has)):
                exp_n, exp = oracle_call(c, ori, has1=has1_now, has2=has2_now)
                n, m = b.resolve(0, has1_now, has2_now)
                assert n == exp_n and np.array_equal(m, exp)
                want = _expected_reeval(c, has1_now, has2_now)
                assert b.reevaluated - seen == want, (b.reevaluated - seen, want)
                seen = b.reevaluated
            assert _expected_reeval(c, c.kf1.has, gained) >= winners[::3].size > 10 and _expected_reeval(c, c.kf1.has, lost) > 100


def test_refusals_leave_the_outputs_untouched(cases):
    store, all_cases = cases
    i = len(all_cases) - 1
    c = all_cases[i]
    n1, n2 = c.kf1.n, c.kf2.n
    k1, k2, off1, off2 = [2 * i], [2 * i + 1], [0, n1], [0, n2]
    epi = ts.pack_epi(c.F12, c.ex, c.ey)
    L = SF.size

    def refused(store_, J, key1, key2, o1, h1, o2, h2, e=epi, nlevels=L, sf=SF, s2=S2, null_out=False):
        table = np.full(n1, 0xDEAD, np.uint32); nq, nm, nd = (np.full(1, -7, np.int32) for _ in range(3))
        rc = ts.pair_eval_host_raw(store_, J, key1, key2, o1, h1, o2, h2, e, nlevels, sf, s2, None if null_out else table, nq, nm, nd)
        assert rc == -1
        assert (table == 0xDEAD).all() and nq[0] == nm[0] == nd[0] == -7
    h1, h2 = c.kf1.has, c.kf2.has
    refused(None, 1, k1, k2, off1, h1, off2, h2)                      # a null store
    refused(store, -1, k1, k2, off1, h1, off2, h2)
    refused(store, 1, [4242], k2, off1, h1, off2, h2)                 # a key that is not live
    refused(store, 1, k1, [4242], off1, h1, off2, h2)
    refused(store, 1, k1, k2, [1, n1 + 1], h1, off2, h2)              # an offset array that does not start at 0
    refused(store, 1, k1, k2, off1, h1, [0, -1], h2)                  # ... that decreases
    refused(store, 1, k1, k2, [0, n1 - 1], h1, off2, h2)              # a mask that is not as long as the keyframe's features
    refused(store, 1, k1, k2, off1, h1, [0, n2 + 1], np.ones(n2 + 1, np.uint8))
    refused(store, 1, k1, k2, off1, None, off2, h2)                   # null masks with a positive length
    refused(store, 1, k1, k2, off1, h1, off2, None)
    refused(store, 1, None, k2, off1, h1, off2, h2)
    refused(store, 1, k1, k2, off1, h1, off2, h2, null_out=True)
    refused(store, 1, k1, k2, off1, h1, off2, h2, e=None)             # a null job_epi
    refused(store, 1, k1, k2, off1, h1, off2, h2, nlevels=0)
    refused(store, 0, k1, k2, off1, h1, off2, h2, nlevels=0)          # nlevels < 1 even without a job
    refused(store, 1, k1, k2, off1, h1, off2, h2, sf=None)
    refused(store, 1, k1, k2, off1, h1, off2, h2, s2=None)
    # a key without a feature vector
    bare = ks.KeyFrameStore(None, 2, 64)
    rng = np.random.default_rng(1)
    kf = Kf(rng.integers(0, 256, (20, 32), dtype=np.uint8), np.zeros(20), np.zeros(20), np.zeros(20), np.zeros(20), fv_of(rng.integers(0, 3, 20)), np.zeros(20))
    add_keyframe(bare, 1, kf); add_keyframe(bare, 2, kf, featvec=False)
    out = (np.zeros(20, np.uint32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32))
    z = np.zeros(20, np.uint8)
    assert ts.pair_eval_host_raw(bare, 1, [1], [2], [0, 20], z, [0, 20], z, epi, L, SF, S2, *out) == -1
    assert ts.pair_eval_host_raw(bare, 1, [1], [1], [0, 20], z, [0, 20], z, epi, L, SF, S2, *out) == 0
    # J == 0 is legal, and so is an octave the tables do not have: the feature is no candidate
    assert ts.pair_eval_host_raw(bare, 0, None, None, None, None, None, None, None, L, SF, S2, None, None, None, None) == 0
    bare.close()


def test_an_octave_beyond_the_tables_is_no_candidate(cases):
    """what ccm_fuse_pose_eval_resident does with such a feature: it is never a candidate and neither table is read for it"""
    store, all_cases = cases
    by = {c.name: (i, c) for i, c in enumerate(all_cases)}
    i, c = by["the den / NaN keyframes on plain rows"]
    full = ts.unpack(ts.pair_eval_host(store, [c.job(2 * i, 2 * i + 1)], SF, S2)["table"])
    assert (full["status"] == 2).all()
    cut = ts.pair_eval_host(store, [c.job(2 * i, 2 * i + 1)], SF[:1], S2[:1])      # every octave is 0: nothing changes
    assert np.array_equal(ts.unpack(cut["table"])["idx"], full["idx"])
    j, c2 = by["dsqr one ulp below the threshold, octave 2"]
    cut = ts.pair_eval_host(store, [c2.job(2 * j, 2 * j + 1)], SF[:2], S2[:2])     # octave 2 with two levels
    assert (ts.unpack(cut["table"])["status"] == 1).all() and cut["n_dist"][0] == 12
