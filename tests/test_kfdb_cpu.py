"""CPU side of the keyframe database: the two restatements of Database.cpp that tests/test_kfdb_gpu.py checks the device against agree, and the
drop-in translation unit shim/Database_hip.cpp compiles against the reference's real class headers and defines every KeyFrameDatabase member."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_kfdb_gpu import RefKeyFrameDatabase, l1_score, phase1_vectorised, place_map, resolve, revisit_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_vectorised_restatement_equals_the_literal_one(seed):
    rng = np.random.default_rng(seed)
    kf_at = place_map(rng, 1500, 10, 80)
    ref = RefKeyFrameDatabase()
    keys, words, values = [], [], []
    for i in range(150):
        w, v = kf_at(int(rng.integers(0, 20)))
        ref.add(i * 7, i % 4, w, v)
        keys.append(i * 7); words.append(w); values.append(v)
    n_rows = 0
    for t in range(20):
        qw, qv = kf_at(int(rng.integers(0, 20)))
        excl = rng.random(len(keys)) < (0.3 if t % 2 else 0.0)
        ex = {k for k, e in zip(keys, excl) if e}
        listed, _, max_common, _, rows = ref.phase1(qw, qv, lambda k: k in ex)
        n_sharing, mc, vrows = phase1_vectorised(keys, words, values, qw, qv, excl)
        assert (n_sharing, mc) == (len(listed), max_common)
        assert [(k, c, float(s32), s) for k, c, s32, s in rows] == [(k, c, float(s32), s) for k, c, s32, s in vrows]
        n_rows += len(rows)
    assert n_rows > 40


def test_l1_score_edge_cases():
    w = np.array([1, 5, 9], np.int32); v = np.array([0.2, 0.3, 0.5])
    assert l1_score(w, v, w, v) == 1.0
    d = l1_score(w, v, np.array([2, 3]), np.array([0.5, 0.5]))
    assert d == 0.0 and np.signbit(d)                        # disjoint: -0.0, as -score/2.0 of a zero sum


def test_resolve_keeps_the_first_best_keyframe_once():
    rows = [(1, 5, np.float32(0.3), 0.3), (2, 5, np.float32(0.5), 0.5), (3, 5, np.float32(0.05), 0.05)]
    out, acc = resolve(rows, 0.1, {1: [2, 9], 2: [1], 3: [2]})
    assert [k for _, k in acc] == [2, 2]                      # key 3 is below minScore; keys 1 and 2 both end at key 2
    assert out == [2]
    kfs, nb, _ = revisit_map()
    assert len(kfs) == 312 and all(len(n) <= 10 for n in nb.values())


@pytest.mark.skipif(not os.path.isdir("/root/reference/cslam"), reason="/root/reference not present (GPU box)")
def test_database_translation_unit_against_the_references_real_headers():
    """shim/Database_hip.cpp compiled to an object against the reference's REAL Database.h / KeyFrame.h / Map.h / Frame.h (make -C shim check_real):
    it defines every cslam::KeyFrameDatabase member that Database.cpp defines, and leaves undefined only members of the reference's own classes."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "shim"), "-s", "check_real"])
    out = subprocess.run(["nm", "-C", os.path.join(ROOT, "shim", "_real", "Database_hip.o")], capture_output=True, text=True, check=True).stdout
    defined = [l.split(" ", 2)[2] for l in out.splitlines() if len(l.split(" ", 2)) == 3 and l.split(" ", 2)[1] in "TW"]
    undefined = [l.strip()[2:] for l in out.splitlines() if l.strip().startswith("U ")]
    for m in ("KeyFrameDatabase(", "add(", "erase(", "clear(", "DetectLoopCandidates(", "DetectMapMatchCandidates(", "DetectRelocalizationCandidates(",
              "AddMP(", "AddDirectBad(", "FindMP(", "FindDirectBad(", "ResetMPs("):
        assert any(d.startswith("cslam::KeyFrameDatabase::" + m) for d in defined), m
    foreign = [u for u in undefined if "cslam::" in u.split("(")[0] and not re.match(r"(.* )?cslam::(KeyFrame|MapPoint|Map|Frame)::", u)]
    assert not foreign, foreign
    assert any(u.startswith("cslam::KeyFrame::GetBestCovisibilityKeyFrames") for u in undefined)   # phase 2 walks the real covisibility graph
    assert any(u.startswith("ccm_kfdb_query") for u in undefined)                                   # phase 1 is the device's
