"""GPU: ccm_bow_pair_eval_resident against the host evaluator, bit for bit (table, n_query, n_dist): every planted case, both frame scenes, no job,
eight jobs that share key1, one candidate key in two jobs under two masks, a keyframe against itself, a keyframe without nodes, work items that do not fill the last
workgroup; the refusals and the lifetime of a slot's feature vector; cslam::SearchByBoWBatch on the device against the oracle, and two threads on one store."""
import threading

import numpy as np
import pytest

import oracle
from bow_search_cases import Kf, add_keyframe, expected_reeval, frame_case, fv_of, install, planted_cases, same_result, same_words
from ccm_slam_amd import bow_search as bs, kfstore as ks, synth

pytestmark = pytest.mark.gpu
E_ARG = -1


@pytest.fixture(scope="module")
def frames():
    o = oracle.OrbOracle(1000)
    out = [o.extract(synth.gen_image(1000, t)) for t in (0, 1)]
    o.close()
    return out


@pytest.fixture(scope="module")
def cases(ctx, frames):
    """every case under its own pair of keys (2 i, 2 i + 1) in one device store, and a keyframe without nodes under the key 1000"""
    all_cases = planted_cases() + [frame_case(frames, 60), frame_case(frames, 6)]
    store = ks.KeyFrameStore(ctx, 2 * len(all_cases) + 4, 1100)
    for i, c in enumerate(all_cases):
        install(store, 2 * i, 2 * i + 1, c)
    rng = np.random.default_rng(3)
    bare = Kf(rng.integers(0, 256, (50, 32), dtype=np.uint8), np.zeros(50), fv_of(-np.ones(50, int)), np.ones(50))
    add_keyframe(store, 1000, bare)
    yield store, all_cases, bare
    store.close()


def both(ctx, store, jobs, tag):
    want = bs.pair_eval_host(store, jobs)
    got = bs.pair_eval_resident(ctx, store, jobs)
    same_result(got, want, tag)
    return got


def test_every_case_alone_and_all_in_one_call(ctx, cases):
    store, all_cases, _ = cases
    for i, c in enumerate(all_cases):
        got = both(ctx, store, [(2 * i, 2 * i + 1, c.kf1.live, c.kf2.live)], c.name)
        same_words(got, got["off"], 0, c, c.name)             # and against the Python replay's reduction
    # the work items of the planted cases: 6, 6, 2, 2 and 2 nodes of keyframe 1, so single calls end in a workgroup of two waves and the joint call does not
    assert [c.kf1.fv[0].size % 4 for c in all_cases[:5]] == [2, 2, 2, 2, 2]
    got = both(ctx, store, [(2 * i, 2 * i + 1, c.kf1.live, c.kf2.live) for i, c in enumerate(all_cases)], "all cases in one call")
    for i, c in enumerate(all_cases):
        same_words(got, got["off"], i, c, (c.name, "in a list"))


def test_job_lists(ctx, cases):
    store, all_cases, bare = cases
    i60, i6 = len(all_cases) - 2, len(all_cases) - 1
    c60, c6 = all_cases[i60], all_cases[i6]
    rng = np.random.default_rng(11)
    # no job
    got = bs.pair_eval_resident(ctx, store, [])
    assert got["table"].size == 0 and got["n_query"].size == 0
    # eight jobs that share key1, the candidates' masks all different; one candidate key in two (here: eight) jobs under different masks
    k1, n1, n2 = 2 * i60, c60.kf1.n, c60.kf2.n
    jobs = [(k1, 2 * i60 + 1, c60.kf1.live, (rng.random(n2) < p).astype(np.uint8)) for p in (0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0, 0.8)]
    got = both(ctx, store, jobs, "eight jobs on one key1")
    assert got["n_query"][0] > 0 and got["n_dist"][0] == 0 and (np.diff(got["n_dist"][:7]) > 0).all()
    # the two frame scenes' keyframes crossed (one key as keyframe 1 of one job and keyframe 2 of another), and a keyframe against itself
    jobs = [(2 * i60, 2 * i6 + 1, c60.kf1.live, c6.kf2.live), (2 * i6 + 1, 2 * i60, c6.kf2.live, c60.kf1.live), (2 * i6, 2 * i6, c6.kf1.live, c6.kf1.live),
            (2 * i60 + 1, 2 * i60 + 1, c60.kf2.live, np.ones(n2, np.uint8))]
    got = both(ctx, store, jobs, "crossed scenes and key1 == key2")
    u = bs.unpack(got["table"][got["off"][2]:got["off"][3]])
    assert (u["d1"][u["status"] == 2] == 0).all() and (u["status"] == 2).sum() > 500
    # a keyframe without nodes: as keyframe 1 (no work item, also alone: nothing is launched), as keyframe 2 (no common node), and between two jobs that have work
    ones = np.ones(50, np.uint8)
    got = both(ctx, store, [(1000, 2 * i60, ones, c60.kf1.live)], "nn == 0 as keyframe 1, alone")
    assert not got["table"].any() and got["n_query"][0] == 0
    got = both(ctx, store, [(k1, 2 * i60 + 1, c60.kf1.live, c60.kf2.live), (1000, 2 * i60, ones, c60.kf1.live), (2 * i60, 1000, c60.kf1.live, ones),
                            (1000, 1000, ones, ones), (k1, 2 * i60 + 1, c60.kf1.live, c60.kf2.live)], "nn == 0 among jobs")
    assert np.array_equal(got["table"][:n1], got["table"][-n1:]) and got["n_query"][[1, 2, 3]].tolist() == [0, 0, 0] and got["n_query"][4] == got["n_query"][0] > 0


def test_refusals_launch_nothing_and_the_next_call_is_right(ctx, cases):
    store, all_cases, _ = cases
    i = len(all_cases) - 2
    c = all_cases[i]
    n1, n2 = c.kf1.n, c.kf2.n
    want = bs.pair_eval_host(store, [(2 * i, 2 * i + 1, c.kf1.live, c.kf2.live)])
    k1, k2 = [2 * i], [2 * i + 1]
    off1, off2 = [0, n1], [0, n2]

    def refused(store_, J, key1, key2, o1, l1, o2, l2, null_out=False):
        table = np.full(n1, 0xDEAD, np.uint64); nq = np.full(1, -7, np.int32); nd = np.full(1, -7, np.int32)
        rc = bs.pair_eval_resident_raw(ctx, store_, J, key1, key2, o1, l1, o2, l2, None if null_out else table, nq, nd)
        assert rc == E_ARG
        assert (table == 0xDEAD).all() and nq[0] == -7 and nd[0] == -7          # nothing written, so nothing ran
        same_result(bs.pair_eval_resident(ctx, store, [(2 * i, 2 * i + 1, c.kf1.live, c.kf2.live)]), want, "the call after a refusal")
    refused(None, 1, k1, k2, off1, c.kf1.live, off2, c.kf2.live)                 # a null store
    refused(store, -1, k1, k2, off1, c.kf1.live, off2, c.kf2.live)
    refused(store, 1, [4242], k2, off1, c.kf1.live, off2, c.kf2.live)            # a key that is not live
    refused(store, 1, k1, [4242], off1, c.kf1.live, off2, c.kf2.live)
    refused(store, 1, k1, k2, [1, n1 + 1], c.kf1.live, off2, c.kf2.live)         # an offset array that does not start at 0
    refused(store, 1, k1, k2, off1, c.kf1.live, [0, -1], c.kf2.live)             # ... that decreases
    refused(store, 1, k1, k2, [0, n1 - 1], c.kf1.live, off2, c.kf2.live)         # a mask that is not as long as the keyframe's features
    refused(store, 1, k1, k2, off1, c.kf1.live, [0, n2 + 1], np.ones(n2 + 1, np.uint8))
    refused(store, 1, k1, k2, off1, None, off2, c.kf2.live)                      # null masks with a positive length
    refused(store, 1, k1, k2, off1, c.kf1.live, off2, None)
    refused(store, 1, None, k2, off1, c.kf1.live, off2, c.kf2.live)
    refused(store, 1, k1, k2, off1, c.kf1.live, off2, c.kf2.live, null_out=True)


def test_a_slots_vector_goes_with_its_tenant(ctx):
    rng = np.random.default_rng(12)

    def mk(n, seed, nodes=4):
        r = np.random.default_rng(seed)
        return Kf(r.integers(0, 256, (n, 32), dtype=np.uint8), np.zeros(n), fv_of(r.integers(0, nodes, n)), np.ones(n))
    a, b, d = mk(40, 1), mk(30, 2), mk(30, 3)
    ones = lambda n: np.ones(n, np.uint8)
    store = ks.KeyFrameStore(ctx, 2, 64)
    add_keyframe(store, 1, a); add_keyframe(store, 2, b, featvec=False)
    out = (np.zeros(40, np.uint64), np.zeros(1, np.int32), np.zeros(1, np.int32))
    raw = lambda k2, n2: bs.pair_eval_resident_raw(ctx, store, 1, [1], [k2], [0, 40], ones(40), [0, n2], ones(n2), *out)
    assert raw(2, 30) == E_ARG                                   # a key without a feature vector
    store.set_featvec(2, b.fv)
    first = both(ctx, store, [(1, 2, ones(40), ones(30))], "after set_featvec")
    assert first["n_query"][0] == 40
    # a second set_featvec replaces the first: other nodes, other answers
    other = fv_of(rng.integers(0, 2, 30))
    store.set_featvec(2, other)
    second = both(ctx, store, [(1, 2, ones(40), ones(30))], "after the second set_featvec")
    assert second["n_dist"][0] != first["n_dist"][0]
    store.set_featvec(2, b.fv)
    same_result(bs.pair_eval_resident(ctx, store, [(1, 2, ones(40), ones(30))]), first, "the first vector again")
    # erase key 2 and put another keyframe into the freed slot WITHOUT a vector: refused, nothing stale is read
    store.erase(2)
    add_keyframe(store, 3, d, featvec=False)
    assert store.count() == (2, 0)
    assert raw(3, 30) == E_ARG and raw(2, 30) == E_ARG
    store.set_featvec(3, d.fv)
    both(ctx, store, [(1, 3, ones(40), ones(30)), (3, 1, ones(30), ones(40))], "the new tenant with its own vector")
    # a refused set_featvec leaves the device vector as it was
    with pytest.raises(ks.StoreError):
        store.set_featvec(3, (d.fv[0], d.fv[1], d.fv[2][::-1].copy()))
    both(ctx, store, [(1, 3, ones(40), ones(30))], "after a refused set_featvec")
    store.clear()
    add_keyframe(store, 1, a, featvec=False)
    assert bs.pair_eval_resident_raw(ctx, store, 1, [1], [1], [0, 40], ones(40), [0, 40], ones(40), *out) == E_ARG
    store.close()


def _oracle(c, nnratio, ori):
    return oracle.search_by_bow_kf_kf(c.kf1.fv, c.kf2.fv, c.kf1.live, c.kf2.live, c.kf1.desc, c.kf1.angle, c.kf2.desc, c.kf2.angle, nnratio, ori)


def test_mirror_on_the_device_against_the_oracle(ctx, cases):
    store, all_cases, _ = cases
    for i in (len(all_cases) - 2, len(all_cases) - 1):
        c = all_cases[i]
        for nnratio, ori in ((0.75, 1), (0.9, 0)):
            exp_n, exp = _oracle(c, nnratio, ori)
            # three candidates in one batch: the scene's keyframe 2 under its own mask, under all ones, and the first planted case's (few common nodes)
            full = np.ones(c.kf2.n, np.uint8)
            p = all_cases[0]
            got = bs.search_by_bow_batch(store, 2 * i, [2 * i + 1, 2 * i + 1, 1], c.kf1.live, [c.kf2.live, full, p.kf2.live], nnratio, ori)
            assert got["nmatches"][0] == exp_n > 100 and np.array_equal(got["matches12"][0], exp), c.name
            host = bs.search_by_bow_batch(store, 2 * i, [2 * i + 1, 2 * i + 1, 1], c.kf1.live, [c.kf2.live, full, p.kf2.live], nnratio, ori, host=True)
            assert got["nmatches"] == host["nmatches"] and all(np.array_equal(a, b) for a, b in zip(got["matches12"], host["matches12"]))
            assert np.array_equal(got["table"], host["table"]) and np.array_equal(got["n_dist"], host["n_dist"]) and got["reevaluated"] == host["reevaluated"]
            single = bs.search_by_bow_batch(store, 2 * i, [2 * i + 1], c.kf1.live, [c.kf2.live], nnratio, ori)
            assert single["reevaluated"] == expected_reeval(c, nnratio) >= 1      # the CPU test's count


def test_two_threads_with_two_contexts_on_one_store(cases):
    store, all_cases, _ = cases
    i = len(all_cases) - 1
    c = all_cases[i]
    want = bs.search_by_bow_batch(store, 2 * i, [2 * i + 1, 2 * i], c.kf1.live, [c.kf2.live, c.kf1.live], 0.75, 1, host=True)
    results, errors = [None, None], []

    def work(t):
        try:
            for _ in range(3):
                results[t] = bs.search_by_bow_batch(store, 2 * i, [2 * i + 1, 2 * i], c.kf1.live, [c.kf2.live, c.kf1.live], 0.75, 1)
        except Exception as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for r in results:
        assert r["nmatches"] == want["nmatches"] and all(np.array_equal(a, b) for a, b in zip(r["matches12"], want["matches12"]))
        assert np.array_equal(r["table"], want["table"]) and r["reevaluated"] == want["reevaluated"]
