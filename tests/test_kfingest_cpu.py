"""CPU: ccm_kfstore_ingest's host evaluator (csrc/kfingest_math.h kfi_ingest_host through the host-only cslam::KeyFrameStore) against the Python replay
of tests/kfingest_cases.py, against oracle.bow_transform and, where it is built, against the reference's own DBoW2; the shadows and grids against add +
set_featvec; every refusal.  Every comparison is exact: integers as integers, doubles as bit patterns."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from ccm_slam_amd import kfstore as ks
from ccm_slam_amd._lib import _p
from kfingest_cases import (MAXF, VEC, by_vocabulary, call_arrays, expected, keyframes, message, planted_properties, same_vectors, vocabularies)
from kfstore_cases import same_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FEAT = VEC + ("feat_word", "feat_node")


def ingest(store, vname, kfs, first_key=1, want_feat=True, angle=True):
    v, levelsup = vocabularies()[vname]
    keys, rec, off, xy, oc, de, ang = call_arrays(kfs, first_key)
    return keys, store.ingest(v, keys, rec, off, xy, oc, de, angle=ang if angle else None, levelsup=levelsup, want_feat=want_feat)


def test_the_constant_is_the_headers():
    txt = open(os.path.join(ROOT, "ccm_slam_amd", "csrc", "kfingest_math.h")).read()
    assert int(re.search(r"#define KFI_MAX_FEAT (\d+)", txt).group(1)) == MAXF >= 4096
    assert f"KFI_MAX_FEAT = {MAXF}" in txt and f"KFI_MAX_FEAT = {MAXF}" in open(os.path.join(ROOT, "include", "ccm_hip.h")).read()


def test_the_planted_keyframes_hold_what_they_are_planted_for():
    planted_properties()


def test_host_evaluator_against_the_replay_every_case_alone():
    for kf in keyframes():
        st = ks.KeyFrameStore(None, 2, MAXF)
        _, got = ingest(st, kf["voc"], [kf])
        same_vectors(got[0], expected(kf), kf["name"], FEAT)
        same_grid(st.get(1), kf["xy"], kf["rec"], kf["name"])
        st.close()


def test_host_evaluator_against_the_replay_all_in_one_call_and_reversed():
    for vname, kfs in by_vocabulary().items():
        for order in (kfs, kfs[::-1], kfs[:3]):
            st = ks.KeyFrameStore(None, len(kfs), MAXF)
            keys, got = ingest(st, vname, order, want_feat=False)
            assert st.count() == (len(order), len(kfs) - len(order))
            for key, kf, g in zip(keys, order, got):
                same_vectors(g, expected(kf), (vname, kf["name"]))
                same_grid(st.get(int(key)), kf["xy"], kf["rec"], kf["name"])
            st.close()


def test_a_full_message_in_one_call():
    kfs = message()
    st = ks.KeyFrameStore(None, 40, 1000)
    _, got = ingest(st, "k10L4", kfs, want_feat=False)
    for kf, g in zip(kfs, got):
        same_vectors(g, expected(kf), kf["name"])
    st.close()


def test_against_the_oracles_transform():
    for name in ("n = 1000", "six on one word", "a negative and a NaN weight", "k7L5, n = 1000", "permuted, n = 257", "cut, n = 1000", "k10L3, n = 64"):
        kf = next(k for k in keyframes() if k["name"] == name)
        v, levelsup = vocabularies()[kf["voc"]]
        word, w, node, bid, bval = oracle.bow_transform(v, kf["desc"], levelsup)
        e = expected(kf)
        assert np.array_equal(word, e["feat_word"]) and np.array_equal(node, e["feat_node"]), name
        assert np.array_equal(bid, e["bow_word"]) and np.array_equal(bval.view(np.uint64), e["bow_value"].view(np.uint64)), name


def test_against_the_references_own_dbow2(tmp_path):
    """ref_bow_transform of oracle/_ref/libmatcher_ref.so (the reference's vendored DBoW2) on a complete tree with the planted weights; skipped where it is not built"""
    path = os.path.join(ROOT, "oracle", "_ref", "libmatcher_ref.so")
    if not os.path.exists(path):
        pytest.skip("oracle/_ref/libmatcher_ref.so is not built")
    import tests.test_ref_matcher as trm
    rlib = C.CDLL(path)
    v, levelsup = vocabularies()["k10L4"]
    if np.isnan(v["weight"]).any():       # the text format carries no NaN: that word goes as stopped, which drops the same features
        v = dict(v); v["weight"] = np.where(np.isnan(v["weight"]), 0.0, v["weight"])
    voc = str(tmp_path / "voc.txt")
    trm._write_orbvoc_txt(voc, v, 10)
    rlib.ref_vocab_load_text.restype = C.c_void_p
    h = rlib.ref_vocab_load_text(voc.encode())
    assert h
    try:
        for kf in [k for k in keyframes() if k["voc"] == "k10L4" and 0 < k["n"] <= 1000]:
            N, desc = kf["n"], kf["desc"]
            ids = np.zeros(N, np.int32); vals = np.zeros(N, np.float64); nfv = np.zeros(1, np.int32)
            fvn = np.zeros(N, np.int32); fvo = np.zeros(N + 1, np.int32); fvf = np.zeros(N, np.int32)
            n = rlib.ref_bow_transform(C.c_void_p(h), _p(desc), N, levelsup, _p(ids), _p(vals), _p(nfv), _p(fvn), _p(fvo), _p(fvf))
            e = expected(kf)
            nn = int(nfv[0])
            got = dict(bow_word=ids[:n], bow_value=vals[:n], fv_node=fvn[:nn], fv_off=fvo[:nn + 1], fv_idx=fvf[:fvo[nn]])
            same_vectors(got, e, kf["name"])
    finally:
        rlib.ref_vocab_free(C.c_void_p(h))


def test_shadows_equal_those_of_add_and_set_featvec():
    for vname, kfs in by_vocabulary().items():
        a, b = ks.KeyFrameStore(None, len(kfs), MAXF), ks.KeyFrameStore(None, len(kfs), MAXF)
        keys, got = ingest(a, vname, kfs)
        _, rec, off, xy, oc, de, ang = call_arrays(kfs)
        b.add(keys, rec, off, xy, oc, de)
        for key, kf, g in zip(keys, kfs, got):
            b.set_featvec(int(key), (g["fv_node"], g["fv_off"], g["fv_idx"]), angle=kf["angle"])
        h = ks._host()
        for key in keys:
            assert h.ccmh_kfstore_shadow_equal(a.handle, b.handle, int(key)) == 1, (vname, int(key))
        a.close(); b.close()


def test_refusals_leave_the_store_and_the_outputs_untouched_and_the_next_call_is_right():
    kfs = [k for k in keyframes() if k["name"] in ("n = 63", "n = 64", "n = 65", "n = 255")]
    big = next(k for k in keyframes() if k["name"] == f"n = {MAXF}")
    v, levelsup = vocabularies()["k10L4"]
    st = ks.KeyFrameStore(None, 4, MAXF + 16)
    ingest(st, "k10L4", kfs[:3])
    before = {k: st.get(k) for k in (1, 2, 3)}
    h = ks._host()

    def refused(code, kfs_, keys, tree=True, null=(), extra=0):
        k0, rec, off, xy, oc, de, ang = call_arrays(kfs_)
        if extra:      # one feature more than KFI_MAX_FEAT
            off = off.copy(); off[-1] += extra
            xy = np.concatenate([xy, xy[:extra]]); oc = np.concatenate([oc, oc[:extra]]); de = np.concatenate([de, de[:extra]])
        out = ks.ingest_outputs(len(keys), int(off[-1]), True)
        for o in out:
            o.view(np.uint8)[:] = 0xA5
        ptr = [None if i in null else _p(o) for i, o in enumerate(out)]
        targs, _alive = ks.tree_args(v)
        if not tree:
            targs = [0, 0] + [None] * 5
        rc = h.ccmh_kfstore_ingest_host(st.handle, *targs, levelsup, len(keys), _p(np.array(keys, np.int64)), _p(rec), _p(off), _p(xy), _p(oc), _p(de), None, *ptr)
        assert rc == code, (keys, rc, code)
        assert all((o.view(np.uint8) == 0xA5).all() for o in out)
        assert st.count() == (3, 1)
        for k, g in before.items():
            now = st.get(k)
            assert now["n"] == g["n"] and np.array_equal(now["cell_off"], g["cell_off"]) and np.array_equal(now["cell_idx"], g["cell_idx"])

    refused(ks.E_STATE, kfs[3:], [3])                       # a live key
    refused(ks.E_STATE, kfs[2:], [9, 9])                    # a key repeated within the call
    refused(ks.E_STATE, kfs[2:], [8, 9])                    # fewer free slots than keyframes
    refused(ks.E_ARG, [big], [9], extra=1)                  # KFI_MAX_FEAT + 1 features (the store would take them)
    refused(ks.E_ARG, kfs[3:], [9], tree=False)             # no vocabulary
    for i in range(7):
        refused(ks.E_ARG, kfs[3:], [9], null=(i,))          # a null output
    refused(ks.E_ARG, kfs[3:], [9], null=(7,))              # feat_word without feat_node
    _, got = ingest(st, "k10L4", kfs[3:], first_key=9)
    same_vectors(got[0], expected(kfs[3]), "after the refusals", FEAT)
    same_grid(st.get(9), kfs[3]["xy"], kfs[3]["rec"], "after the refusals")
    # KFI_MAX_FEAT itself is taken
    st.erase(9)
    _, got = ingest(st, "k10L4", [big], first_key=10)
    same_vectors(got[0], expected(big), big["name"], FEAT)
    st.close()


def test_m_zero_and_empty_keyframes():
    st = ks.KeyFrameStore(None, 3, 64)
    v, levelsup = vocabularies()["k10L4"]
    assert st.ingest(v, [], None, None, None, None, None) == []
    empty = next(k for k in keyframes() if k["name"] == "n = 0")
    keys, got = ingest(st, "k10L4", [empty, empty], first_key=5)
    for g in got:
        same_vectors(g, expected(empty), "n = 0")
        assert g["bow_word"].size == 0 and np.array_equal(g["fv_off"], [0])
    assert st.count() == (2, 1) and st.get(5)["n"] == 0
    st.close()


def test_the_cpp_mirror_with_a_vocabulary_without_a_context(tmp_path):
    """tests/host/kfingest_mirror_check.cpp against libccm_host.so: cslam::ORBVocabulary constructed without a context and cslam::KeyFrameStore::ingest with
    std::vector<BowVector> / std::vector<FeatureVector> on a host-only store, the route INTEGRATION.md §7q names"""
    import subprocess
    pkg = os.path.join(ROOT, "ccm_slam_amd")
    exe = tmp_path / "kfingest_mirror_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", str(exe),
                    os.path.join(ROOT, "tests", "host", "kfingest_mirror_check.cpp"), "-L", pkg, "-lccm_host", "-lccm_hip", f"-Wl,-rpath,{pkg}",
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("kfingest mirror ok"), (r.stdout[-2000:], r.stderr[-2000:])
