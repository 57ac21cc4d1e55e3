"""GPU: ccm_kfstore_ingest against the host evaluator and the Python replay of tests/kfingest_cases.py, bit for bit: every planted keyframe alone,
all of a vocabulary in one call and in reverse order, a full message; the per-feature words and nodes against ccm_bow_transform; the slot's grid and feature vector
and the resident consumers against a second store filled by add + set_featvec; ccm_kfdb_add on every BowVector; the refusals; slot reuse; the mirror; threads."""
import ctypes as C
import threading

import numpy as np
import pytest

from ccm_slam_amd import bow_search as bs, kfdb, kfstore as ks, matcher, synth, tri_search as ts
from ccm_slam_amd._lib import Context, _p, hooks
from kfingest_cases import MAXF, VEC, by_vocabulary, call_arrays, expected, keyframes, message, same_vectors, vocabularies
from kfstore_cases import same_grid

pytestmark = pytest.mark.gpu
FEAT = VEC + ("feat_word", "feat_node")
SLOTS = 48


@pytest.fixture(scope="module")
def vocs(ctx):
    out = {name: matcher.Vocabulary(ctx, v) for name, (v, _) in vocabularies().items()}
    yield out
    for v in out.values():
        v.close()


@pytest.fixture(scope="module")
def store(ctx):
    st = ks.KeyFrameStore(ctx, SLOTS, MAXF + 16)
    yield st
    st.close()


@pytest.fixture(scope="module")
def host_vectors():
    """the host evaluator's vectors of every keyframe (the host-only store), computed once"""
    out = {}
    for vname, kfs in list(by_vocabulary().items()) + [("k10L4", message())]:
        st = ks.KeyFrameStore(None, len(kfs), MAXF)
        keys, rec, off, xy, oc, de, ang = call_arrays(kfs)
        v, levelsup = vocabularies()[vname]
        for kf, g in zip(kfs, st.ingest(v, keys, rec, off, xy, oc, de, levelsup=levelsup, want_feat=True)):
            out[kf["name"]] = g
        st.close()
    return out


def ingest(st, vocs, vname, kfs, first_key=1, want_feat=True, angle=True):
    keys, rec, off, xy, oc, de, ang = call_arrays(kfs, first_key)
    return keys, st.ingest(vocs[vname], keys, rec, off, xy, oc, de, angle=ang if angle else None, levelsup=vocabularies()[vname][1], want_feat=want_feat)


def slot_featvec(ctx, st, key, n):
    """the key's feature vector as its slot holds it (the test hook), or None"""
    h = hooks()
    nn = C.c_int(-7)
    node, off, idx = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    assert h.ccm_kfstore_debug_get_featvec(st.raw, ctx.handle, int(key), C.byref(nn), _p(node), _p(off), _p(idx)) == 0
    if nn.value < 0:
        return None
    off = off[:nn.value + 1] if nn.value else np.zeros(1, np.int32)
    return dict(fv_node=node[:nn.value].copy(), fv_off=off.copy(), fv_idx=idx[:int(off[-1])].copy())


def test_every_case_alone_against_the_host_evaluator_and_the_replay(ctx, vocs, store, host_vectors):
    for kf in keyframes():
        store.clear()
        _, got = ingest(store, vocs, kf["voc"], [kf])
        same_vectors(got[0], host_vectors[kf["name"]], kf["name"], FEAT)
        same_vectors(got[0], expected(kf), (kf["name"], "replay"), FEAT)
        same_grid(store.get(1), kf["xy"], kf["rec"], kf["name"])
        same_vectors(slot_featvec(ctx, store, 1, kf["n"]), expected(kf), (kf["name"], "slot"), ("fv_node", "fv_off", "fv_idx"))


def test_all_in_one_call_and_in_reverse_order(ctx, vocs, store, host_vectors):
    for vname, kfs in by_vocabulary().items():
        for order in (kfs, kfs[::-1]):
            store.clear()
            keys, got = ingest(store, vocs, vname, order, want_feat=False)
            assert store.count() == (len(order), SLOTS - len(order))
            for key, kf, g in zip(keys, order, got):
                same_vectors(g, host_vectors[kf["name"]], (vname, kf["name"]))
                same_grid(store.get(int(key)), kf["xy"], kf["rec"], kf["name"])
                same_vectors(slot_featvec(ctx, store, key, kf["n"]), expected(kf), (kf["name"], "slot"), ("fv_node", "fv_off", "fv_idx"))


def test_a_full_message_and_three_keyframes(ctx, vocs, store, host_vectors):
    kfs = message()
    for part in (kfs, kfs[:3]):
        store.clear()
        keys, got = ingest(store, vocs, "k10L4", part, want_feat=False)
        for key, kf, g in zip(keys, part, got):
            same_vectors(g, host_vectors[kf["name"]], kf["name"])
        same_grid(store.get(int(keys[-1])), part[-1]["xy"], part[-1]["rec"], "the last of the message")


def test_the_per_feature_results_are_bow_transforms(ctx, vocs, store):
    for name in ("n = 1000", "n = 1025", "cut, n = 1000", "k10L3, n = 257", "k7L5, n = 257", "permuted, n = 1000"):
        kf = next(k for k in keyframes() if k["name"] == name)
        store.clear()
        _, with_ = ingest(store, vocs, kf["voc"], [kf], want_feat=True)
        store.clear()
        _, without = ingest(store, vocs, kf["voc"], [kf], want_feat=False)
        assert "feat_word" not in without[0]
        same_vectors(without[0], with_[0], name)
        word, w, node = vocs[kf["voc"]].transform(kf["desc"], vocabularies()[kf["voc"]][1])[:3]
        assert np.array_equal(with_[0]["feat_word"], word) and np.array_equal(with_[0]["feat_node"], node), name


@pytest.fixture(scope="module")
def twin(ctx, vocs, host_vectors):
    """the message's first eight keyframes under the keys 1 .. 8 in two device stores: one ingested, one filled by add + set_featvec from the host evaluator's vectors"""
    kfs = message()[:8]
    a, b = ks.KeyFrameStore(ctx, 8, 1000), ks.KeyFrameStore(ctx, 8, 1000)
    keys, got = ingest(a, vocs, "k10L4", kfs)
    _, rec, off, xy, oc, de, ang = call_arrays(kfs)
    b.add(keys, rec, off, xy, oc, de)
    for key, kf in zip(keys, kfs):
        g = host_vectors[kf["name"]]
        b.set_featvec(int(key), (g["fv_node"], g["fv_off"], g["fv_idx"]), angle=kf["angle"])
    yield a, b, kfs, got
    a.close(); b.close()


def test_slot_and_shadow_equal_those_of_add_and_set_featvec(ctx, twin):
    a, b, kfs, _ = twin
    h = ks._host()
    for key, kf in enumerate(kfs, 1):
        ga, gb = a.get(key), b.get(key)
        assert ga["n"] == gb["n"] and ga["n_in"] == gb["n_in"] and np.array_equal(ga["cell_off"], gb["cell_off"]) and np.array_equal(ga["cell_idx"], gb["cell_idx"])
        same_vectors(slot_featvec(ctx, a, key, kf["n"]), slot_featvec(ctx, b, key, kf["n"]), key, ("fv_node", "fv_off", "fv_idx"))
        assert h.ccmh_kfstore_shadow_equal(a.handle, b.handle, key) == 1


def test_the_resident_consumers_agree(ctx, twin):
    a, b, kfs, _ = twin
    rng = np.random.default_rng(5)
    live = [(rng.random(k["n"]) < 0.8).astype(np.uint8) for k in kfs]
    jobs = [(1, j, live[0], live[j - 1]) for j in range(2, 9)] + [(3, 3, live[2], live[2])]
    ra, rb = bs.pair_eval_resident(ctx, a, jobs), bs.pair_eval_resident(ctx, b, jobs)
    for f in ("table", "n_query", "n_dist"):
        assert np.array_equal(ra[f], rb[f]), f
    assert ra["n_dist"].sum() > 0
    sf, _, s2, _ = synth.scale_tables()
    has = [(rng.random(k["n"]) < 0.5).astype(np.uint8) for k in kfs]
    tj = [(1, j, has[0], has[j - 1]) + ts.epipolar_of(synth.EUROC_K, np.array([-0.1 - 0.01 * j, 0.01, 0.02], np.float32)) for j in range(2, 9)]
    ta, tb = ts.pair_eval_resident(ctx, a, tj, sf, s2), ts.pair_eval_resident(ctx, b, tj, sf, s2)
    for f in ("table", "n_query", "n_match", "n_dist"):
        assert np.array_equal(ta[f], tb[f]), f
    assert ta["n_dist"].sum() > 0


def test_the_keyframe_database_accepts_every_bow_vector(ctx, host_vectors, vocs, store):
    for vname, kfs in by_vocabulary().items():
        store.clear()
        _, got = ingest(store, vocs, vname, kfs, want_feat=False)
        db = kfdb.KeyFrameDatabase(ctx, int(vocabularies()[vname][0]["word_id"].max()) + 1)
        for key, g in enumerate(got):
            db.add(key, 0, g["bow_word"], g["bow_value"])
        db.close()


def test_refusals_leave_the_store_and_the_outputs_untouched_and_the_next_call_is_right(ctx, vocs):
    kfs = [k for k in keyframes() if k["name"] in ("n = 63", "n = 64", "n = 65", "n = 255")]
    big = next(k for k in keyframes() if k["name"] == f"n = {MAXF}")
    st = ks.KeyFrameStore(ctx, 4, MAXF + 16)
    ingest(st, vocs, "k10L4", kfs[:3])
    before = {k: (st.get(k), slot_featvec(ctx, st, k, kfs[k - 1]["n"])) for k in (1, 2, 3)}
    h = ks._host()

    def refused(code, kfs_, keys, voc=True, null=(), extra=0):
        _, rec, off, xy, oc, de, ang = call_arrays(kfs_)
        if extra:      # one feature more than KFI_MAX_FEAT
            off = off.copy(); off[-1] += extra
            xy = np.concatenate([xy, xy[:extra]]); oc = np.concatenate([oc, oc[:extra]]); de = np.concatenate([de, de[:extra]])
        out = ks.ingest_outputs(len(keys), int(off[-1]), True)
        for o in out:
            o.view(np.uint8)[:] = 0xA5
        ptr = [None if i in null else _p(o) for i, o in enumerate(out)]
        rc = h.ccmh_kfstore_ingest(st.handle, st.device, vocs["k10L4"]._h if voc else None, 2, len(keys), _p(np.array(keys, np.int64)), _p(rec), _p(off), _p(xy), _p(oc),
                                   _p(de), None, *ptr)
        assert rc == code, (keys, rc, code)
        assert all((o.view(np.uint8) == 0xA5).all() for o in out)
        assert st.count() == (3, 1)
        for k, (g, fv) in before.items():
            now = st.get(k)
            assert now["n"] == g["n"] and np.array_equal(now["cell_off"], g["cell_off"]) and np.array_equal(now["cell_idx"], g["cell_idx"])
            same_vectors(slot_featvec(ctx, st, k, g["n"]), fv, k, ("fv_node", "fv_off", "fv_idx"))

    refused(ks.E_STATE, kfs[3:], [3])                       # a live key
    refused(ks.E_STATE, kfs[2:], [9, 9])                    # a key repeated within the call
    refused(ks.E_STATE, kfs[2:], [8, 9])                    # fewer free slots than keyframes
    refused(ks.E_ARG, [big], [9], extra=1)                  # KFI_MAX_FEAT + 1 features (the store would take them)
    refused(ks.E_ARG, kfs[3:], [9], voc=False)              # no vocabulary
    for i in range(7):
        refused(ks.E_ARG, kfs[3:], [9], null=(i,))          # a null output
    refused(ks.E_ARG, kfs[3:], [9], null=(8,))              # feat_node without feat_word's partner
    _, got = ingest(st, vocs, "k10L4", kfs[3:], first_key=9)
    same_vectors(got[0], expected(kfs[3]), "after the refusals", FEAT)
    same_grid(st.get(9), kfs[3]["xy"], kfs[3]["rec"], "after the refusals")
    st.close()


def test_slot_reuse_set_featvec_after_ingest_and_m_zero(ctx, vocs):
    kf = {k["name"]: k for k in keyframes()}
    st = ks.KeyFrameStore(ctx, 2, 1100)
    assert st.ingest(vocs["k10L4"], [], None, None, None, None, None) == [] and st.count() == (0, 2)
    ingest(st, vocs, "k10L4", [kf["n = 1000"], kf["n = 257"]])
    st.erase(1)
    assert st.count() == (1, 1)
    small = kf["stopped among kept"]      # fewer features than the slot's previous tenant
    _, got = ingest(st, vocs, "k10L4", [small], first_key=7)
    same_vectors(got[0], expected(small), "reused slot", FEAT)
    same_grid(st.get(7), small["xy"], small["rec"], "reused slot")
    same_vectors(slot_featvec(ctx, st, 7, small["n"]), expected(small), "reused slot", ("fv_node", "fv_off", "fv_idx"))
    same_vectors(slot_featvec(ctx, st, 2, 257), expected(kf["n = 257"]), "the neighbour", ("fv_node", "fv_off", "fv_idx"))
    # set_featvec after ingest replaces the vector
    fv = (np.array([4, 9], np.int32), np.array([0, 2, 3], np.int32), np.array([1, 5, 0], np.int32))
    st.set_featvec(7, fv)
    same_vectors(slot_featvec(ctx, st, 7, small["n"]), dict(fv_node=fv[0], fv_off=fv[1], fv_idx=fv[2]), "replaced", ("fv_node", "fv_off", "fv_idx"))
    # a keyframe whose words are all stopped has an empty vector, not none
    st.erase(7)
    ingest(st, vocs, "k10L4", [kf["every word stopped"]], first_key=8)
    got = slot_featvec(ctx, st, 8, kf["every word stopped"]["n"])
    assert got is not None and got["fv_node"].size == 0
    st.close()


def test_the_mirror_on_the_device_against_the_host_mirror(ctx, vocs):
    h = ks._host()
    for vname, kfs in by_vocabulary().items():
        kfs = [k for k in kfs if k["n"] <= 1025]
        a, b = ks.KeyFrameStore(ctx, len(kfs), 1025), ks.KeyFrameStore(None, len(kfs), 1025)
        keys, ga = ingest(a, vocs, vname, kfs)
        keys2, rec, off, xy, oc, de, ang = call_arrays(kfs)
        gb = b.ingest(vocabularies()[vname][0], keys2, rec, off, xy, oc, de, angle=ang, levelsup=vocabularies()[vname][1], want_feat=True)
        for key, x, y in zip(keys, ga, gb):
            same_vectors(x, y, (vname, int(key)), FEAT)
            assert h.ccmh_kfstore_shadow_equal(a.handle, b.handle, int(key)) == 1, (vname, int(key))
        a.close(); b.close()


def test_two_threads_ingest_while_a_third_searches(ctx, vocs, host_vectors):
    """ONE store: the keys 1 .. 8 are ingested first; then two threads with their own contexts ingest (and erase, and ingest again) disjoint other keys into the free
    slots of that store while a third thread with its own context runs the resident search on the keys 1 .. 8.  Every table equals the one taken alone, every
    vector the host evaluator's, and the searched keys' slots are what they were."""
    msg = message()
    st = ks.KeyFrameStore(ctx, 20, 1000)
    first = msg[:8]
    ingest(st, vocs, "k10L4", first, first_key=1, want_feat=False)
    live = [np.ones(k["n"], np.uint8) for k in first]
    jobs = [(1, j, live[0], live[j - 1]) for j in range(2, 9)]
    want = bs.pair_eval_resident(ctx, st, jobs)
    assert want["n_dist"].sum() > 0
    slots = {k: (st.get(k), slot_featvec(ctx, st, k, 1000)) for k in range(1, 9)}
    results, errors = {}, []
    ROUNDS = 4      # bounded, whatever the other threads do

    def ingester(t):
        try:
            part = msg[10 + 10 * t:10 + 10 * t + 6]
            k0 = 100 * (t + 1)
            for r in range(ROUNDS):
                results[(t, r)] = (ingest(st, vocs, "k10L4", part[:3], first_key=k0, want_feat=False)[1] +
                                   ingest(st, vocs, "k10L4", part[3:], first_key=k0 + 3, want_feat=False)[1])
                if r + 1 < ROUNDS:      # the slots go back and are taken again, by whichever thread comes first
                    for k in range(k0, k0 + 6):
                        st.erase(k)
        except BaseException as e:      # noqa: BLE001
            errors.append(e)

    def searcher():
        try:
            c = Context(0)
            try:
                for r in range(12):
                    results[("s", r)] = bs.pair_eval_resident(c, st, jobs)
            finally:
                c.close()
        except BaseException as e:      # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=ingester, args=(t,)) for t in range(2)] + [threading.Thread(target=searcher)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for t in range(2):
        for r in range(ROUNDS):
            for kf, g in zip(msg[10 + 10 * t:10 + 10 * t + 6], results[(t, r)]):
                same_vectors(g, host_vectors[kf["name"]], (t, r, kf["name"]))
    for r in range(12):
        for f in ("table", "n_query", "n_dist"):
            assert np.array_equal(results[("s", r)][f], want[f]), (r, f)
    assert st.count() == (20, 0)
    for k, (g, fv) in slots.items():      # the searched keys' slots are untouched by the ingests beside them
        now = st.get(k)
        assert now["n_in"] == g["n_in"] and np.array_equal(now["cell_off"], g["cell_off"]) and np.array_equal(now["cell_idx"], g["cell_idx"])
        same_vectors(slot_featvec(ctx, st, k, 1000), fv, k, ("fv_node", "fv_off", "fv_idx"))
    for t in range(2):      # and the ingested ones hold their own
        for i in (0, 5):
            kf = msg[10 + 10 * t + i]
            same_vectors(slot_featvec(ctx, st, 100 * (t + 1) + i, 1000), expected(kf), (t, i), ("fv_node", "fv_off", "fv_idx"))
            same_grid(st.get(100 * (t + 1) + i), kf["xy"], kf["rec"], (t, i))
    after = bs.pair_eval_resident(ctx, st, jobs)
    assert np.array_equal(after["table"], want["table"])
    st.close()
