"""GPU: ccm_tri_search_eval_resident against the host evaluator, bit for bit (table, n_query, n_match, n_dist): every planted case and the frame scene
alone (the last workgroup then holds one to three waves) and all in one call, no job, twenty jobs that share key1 with their own F12 and masks, a keyframe against
itself, a keyframe without nodes; the refusals and the lifetime of a slot's feature vector; cslam::SearchForTriangulationBatch on the device against the oracle and
the host mirror through a 6-neighbour sequence, and two threads on one store."""
import threading

import numpy as np
import pytest

import oracle
from tri_search_cases import (S2, SF, Kf, add_keyframe, frame_case, fv_of, install, install_sequence, planted_cases, run_sequence, same_result, same_words, sequence_cases)
from ccm_slam_amd import kfstore as ks, synth, tri_search as ts

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
    all_cases = planted_cases() + [frame_case(frames)]
    store = ks.KeyFrameStore(ctx, 2 * len(all_cases) + 4, 1100)
    for i, c in enumerate(all_cases):
        install(store, 2 * i, 2 * i + 1, c)
    rng = np.random.default_rng(3)
    z = np.zeros(50)
    bare = Kf(rng.integers(0, 256, (50, 32), dtype=np.uint8), z + 10, z + 100, z, z, fv_of(-np.ones(50, int)), z)
    add_keyframe(store, 1000, bare)
    yield store, all_cases, bare
    store.close()


@pytest.fixture(scope="module")
def sequence(frames):
    return sequence_cases(frames)


def both(ctx, store, jobs, tag):
    want = ts.pair_eval_host(store, jobs, SF, S2)
    got = ts.pair_eval_resident(ctx, store, jobs, SF, S2)
    same_result(got, want, tag)
    return got


def test_every_case_alone_and_all_in_one_call(ctx, cases):
    store, all_cases, _ = cases
    for i, c in enumerate(all_cases):
        got = both(ctx, store, [c.job(2 * i, 2 * i + 1)], c.name)
        same_words(got, got["off"], 0, c, c.name)             # and against the Python replay
    # a single call's work items are the nodes of its keyframe 1: the last workgroup holds one, two and three waves among the planted cases
    assert {c.kf1.fv[0].size % 4 for c in all_cases[:-1]} >= {1, 2, 3}
    got = both(ctx, store, [c.job(2 * i, 2 * i + 1) for i, c in enumerate(all_cases)], "all cases in one call")
    for i, c in enumerate(all_cases):
        same_words(got, got["off"], i, c, (c.name, "in a list"))


def test_job_lists(ctx, cases):
    store, all_cases, bare = cases
    i = len(all_cases) - 1
    c = all_cases[i]
    n1, n2 = c.kf1.n, c.kf2.n
    rng = np.random.default_rng(11)
    # no job
    got = ts.pair_eval_resident(ctx, store, [], SF, S2)
    assert got["table"].size == 0 and got["n_query"].size == 0
    # twenty jobs that share key1, every job with its own F12, epipole and masks (one of them with every candidate taken: nothing to count)
    jobs = []
    for j in range(20):
        F = (c.F12 * np.float32(1 + 0.02 * j)).astype(np.float32); F[5] += np.float32(1e-7 * j)
        jobs.append((2 * i, 2 * i + 1, (rng.random(n1) < 0.05 * j).astype(np.uint8), (rng.random(n2) < (1.0 if j == 7 else 0.04 * j)).astype(np.uint8), F,
                     c.ex + np.float32(5 * j), c.ey - np.float32(3 * j)))
    got = both(ctx, store, jobs, "twenty jobs on one key1")
    assert got["n_match"][0] > 40 and got["n_dist"][7] == 0 and got["n_match"][7] == 0 and got["n_query"][7] > 0
    assert len({got["table"][got["off"][j]:got["off"][j + 1]].tobytes() for j in range(20)}) == 20
    # a keyframe against itself without any map point and on its own rows (F12 of a sideways motion, the epipole far away): every query finds a candidate at distance 0
    none1 = np.zeros(n1, np.uint8)
    got = both(ctx, store, [(2 * i, 2 * i, none1, none1, c.F12, c.ex, c.ey), (2 * i + 1, 2 * i, c.kf2.has, c.kf1.has, c.F12, c.ex, c.ey)],
               "key1 == key2, and the scene's keys crossed")
    u = ts.unpack(got["table"][:n1])
    assert (u["status"] == 2).sum() > 900 and (u["dist"][u["status"] == 2] == 0).all()
    # a keyframe without nodes: as keyframe 1 (no work item, also alone: nothing is launched), as keyframe 2 (no common node), and between two jobs that have work
    zeros = np.zeros(50, np.uint8)
    got = both(ctx, store, [(1000, 2 * i, zeros, c.kf1.has, c.F12, c.ex, c.ey)], "nn == 0 as keyframe 1, alone")
    assert not got["table"].any() and got["n_query"][0] == 0
    got = both(ctx, store, [c.job(2 * i, 2 * i + 1), (1000, 2 * i, zeros, c.kf1.has, c.F12, c.ex, c.ey), (2 * i, 1000, c.kf1.has, zeros, c.F12, c.ex, c.ey),
                            (1000, 1000, zeros, zeros, c.F12, c.ex, c.ey), c.job(2 * i, 2 * i + 1)], "nn == 0 among jobs")
    assert np.array_equal(got["table"][:n1], got["table"][-n1:]) and got["n_query"][[1, 2, 3]].tolist() == [0, 0, 0] and got["n_query"][4] == got["n_query"][0] > 0


def test_refusals_launch_nothing_and_the_next_call_is_right(ctx, cases):
    store, all_cases, _ = cases
    i = len(all_cases) - 1
    c = all_cases[i]
    n1, n2 = c.kf1.n, c.kf2.n
    want = ts.pair_eval_host(store, [c.job(2 * i, 2 * i + 1)], SF, S2)
    k1, k2, off1, off2 = [2 * i], [2 * i + 1], [0, n1], [0, n2]
    epi = ts.pack_epi(c.F12, c.ex, c.ey)
    L = SF.size

    def refused(store_, J, key1, key2, o1, h1, o2, h2, e=epi, nlevels=L, sf=SF, s2=S2, null_out=False):
        table = np.full(n1, 0xDEAD, np.uint32); nq, nm, nd = (np.full(1, -7, np.int32) for _ in range(3))
        rc = ts.pair_eval_resident_raw(ctx, store_, J, key1, key2, o1, h1, o2, h2, e, nlevels, sf, s2, None if null_out else table, nq, nm, nd)
        assert rc == E_ARG
        assert (table == 0xDEAD).all() and nq[0] == nm[0] == nd[0] == -7          # nothing written, so nothing ran
        same_result(ts.pair_eval_resident(ctx, store, [c.job(2 * i, 2 * i + 1)], SF, S2), want, "the call after a refusal")
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
    refused(store, 1, k1, k2, off1, h1, off2, h2, null_out=True)      # a null table
    refused(store, 1, k1, k2, off1, h1, off2, h2, e=None)             # a null job_epi
    refused(store, 1, k1, k2, off1, h1, off2, h2, nlevels=0)
    refused(store, 0, k1, k2, off1, h1, off2, h2, nlevels=0)
    refused(store, 1, k1, k2, off1, h1, off2, h2, sf=None)
    refused(store, 1, k1, k2, off1, h1, off2, h2, s2=None)


def test_a_slots_vector_goes_with_its_tenant(ctx):
    def mk(n, seed, nodes=4):
        r = np.random.default_rng(seed)
        z = np.zeros(n)
        return Kf(r.integers(0, 256, (n, 32), dtype=np.uint8), r.uniform(20, 700, n), z + 100, z, z, fv_of(r.integers(0, nodes, n)), z)
    a, b, d = mk(40, 1), mk(30, 2), mk(30, 3)
    b.desc[:10] = a.desc[:10]; d.desc[:10] = a.desc[10:20]               # some matches either way
    F, ex, ey = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32), np.float32(-1000), np.float32(240)
    zeros = lambda n: np.zeros(n, np.uint8)
    store = ks.KeyFrameStore(ctx, 2, 64)
    add_keyframe(store, 1, a); add_keyframe(store, 2, b, featvec=False)
    out = (np.zeros(40, np.uint32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32))
    epi = ts.pack_epi(F, ex, ey)
    raw = lambda k2, n2: ts.pair_eval_resident_raw(ctx, store, 1, [1], [k2], [0, 40], zeros(40), [0, n2], zeros(n2), epi, SF.size, SF, S2, *out)
    assert raw(2, 30) == E_ARG                                   # a key without a feature vector
    store.set_featvec(2, b.fv)
    first = both(ctx, store, [(1, 2, zeros(40), zeros(30), F, ex, ey)], "after set_featvec")
    assert first["n_query"][0] == 40
    # erase key 2 and put another keyframe into the freed slot WITHOUT a vector: refused, nothing stale is read
    store.erase(2)
    add_keyframe(store, 3, d, featvec=False)
    assert store.count() == (2, 0)
    assert raw(3, 30) == E_ARG and raw(2, 30) == E_ARG
    store.set_featvec(3, d.fv)
    second = both(ctx, store, [(1, 3, zeros(40), zeros(30), F, ex, ey), (3, 1, zeros(30), zeros(40), F, ex, ey)], "the new tenant with its own vector")
    assert not np.array_equal(second["table"][:40], first["table"])
    store.close()


def test_mirror_on_the_device_through_the_sequence(ctx, sequence):
    seq, has1 = sequence
    store = ks.KeyFrameStore(ctx, 8, 1100)
    install_sequence(store, seq)
    total_d, tab_d = run_sequence(store, seq, has1, host=False)          # every call against the oracle's single call on the flags of its moment
    total_h, tab_h = run_sequence(store, seq, has1, host=True)
    assert total_d == total_h > 100
    same_result(tab_d, tab_h, "the device batch's table against the host batch's")
    total_o, _ = run_sequence(store, seq, has1, host=False, ori=1)
    assert total_o > 100
    store.close()


def test_two_threads_with_two_contexts_on_one_store(cases):
    store, all_cases, _ = cases
    i = len(all_cases) - 1
    c = all_cases[i]
    args = (store, 2 * i, [2 * i + 1, 2 * i], c.kf1.has, [c.kf2.has, c.kf1.has], [(c.F12, c.ex, c.ey)] * 2, S2, SF, 1)
    want = ts.search_for_triangulation_batch(*args, host=True)
    results, errors = [None, None], []

    def work(t):
        try:
            for _ in range(3):
                results[t] = ts.search_for_triangulation_batch(*args)
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
        same_result(r, want, "a thread's batch")
