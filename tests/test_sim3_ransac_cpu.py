"""CPU side of the Sim3 RANSAC: known answers for the restated OpenCV primitives of the checker (tests/test_sim3_ransac_gpu.py), the RANSAC
parameters and draws of Sim3Solver.cpp, the per-hypothesis lines of sim3_ransac_math.h compiled for the host against the checker, and the batched
schedule of ccm_slam_amd/host/sim3_schedule.h against a literal round-robin (tests/host/sim3_schedule_check.cpp)."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from test_sim3_ransac_gpu import (ArrayDraw, compute_sim3, jacobi, max_error_thresholds, random_int, ransac_max_iterations, ref_compute_sim3,
                                  ref_hypothesis, rodrigues, sample_indices)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _rot(w):
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def test_exact_similarity_is_recovered():
    rng = np.random.default_rng(0)
    for fix in (False, True):
        R = _rot(np.array([0.1, -0.2, 0.15]))
        s = 1.0 if fix else 1.3
        t = np.array([0.3, -0.1, 0.2])
        X2 = rng.uniform(-1, 1, (3, 3)) + [0, 0, 4]
        X1 = s * X2 @ R.T + t
        h = compute_sim3(X1.astype(np.float32), X2.astype(np.float32), fix)
        assert np.abs(h["R"] - R).max() < 2e-5
        assert abs(h["s"] - s) < 2e-5
        assert np.abs(h["t"] - t).max() < 1e-4
        # the two transforms of CheckInliers are inverse to each other
        S12 = np.eye(4); S12[:3, :3] = h["sR"]; S12[:3, 3] = h["t"]
        S21 = np.eye(4); S21[:3, :3] = h["sRi"]; S21[:3, 3] = h["ti"]
        assert np.abs(S12 @ S21 - np.eye(4)).max() < 1e-5


def test_jacobi_matches_eigh_up_to_sign():
    rng = np.random.default_rng(1)
    for _ in range(20):
        A = rng.normal(size=(4, 4)).astype(np.float32)
        A = (A + A.T).astype(np.float32)
        W, V = jacobi(A)
        w, v = np.linalg.eigh(A.astype(np.float64))
        assert np.all(np.diff(W) <= 0)                                   # descending, eigenvectors as rows
        assert np.abs(W - w[::-1]).max() < 1e-5 * max(1, np.abs(w).max())
        for i in range(4):
            e = v[:, 3 - i]
            assert min(np.abs(V[i] - e).max(), np.abs(V[i] + e).max()) < 1e-4
    W, V = jacobi(np.diag([1.0, 3.0, 2.0, 3.0]).astype(np.float32))       # no rotation; a tie keeps its first index
    assert list(W) == [3, 3, 2, 1] and list(np.argmax(np.abs(V), 1)) == [1, 3, 2, 0]


def test_rodrigues_matches_its_closed_form():
    for w in ([0.3, -0.2, 0.1], [1e-3, 2e-3, -1e-3], [2.5, 0.5, -1.0]):
        w = np.array(w, np.float32)
        assert np.abs(rodrigues(w) - _rot(w.astype(np.float64))).max() < 1e-6
    assert np.array_equal(rodrigues(np.zeros(3, np.float32)), np.eye(3, dtype=np.float32))
    assert np.isnan(rodrigues(np.array([np.nan, 0, 0], np.float32))).all()


def test_duplicated_sample_gives_nan():
    x = np.array([[1, 2, 5], [1, 2, 5], [1, 2, 5]], np.float32)
    h = compute_sim3(x, x, False)
    assert np.isnan(h["R"]).all() and np.isnan(h["t"]).all()


def test_threshold_table():
    from ccm_slam_amd import sim3, synth
    _, _, s2, _ = synth.scale_tables()
    assert list(max_error_thresholds(s2)) == [9, 13, 19, 27, 39, 57, 82, 118]
    assert np.array_equal(sim3.max_error_thresholds(s2), max_error_thresholds(s2))


def test_iteration_bound():
    assert [ransac_max_iterations(N) for N in (6, 7, 20, 24, 25)] == [1, 5, 169, 293, 300]


def test_draws_to_indices():
    # raw values chosen at known fractions of RAND_MAX + 1: randi = floor(frac * size)
    q = lambda frac: int(frac * 2147483648.0)
    assert sample_indices([q(0.0), q(0.0), q(0.0)], 10) == [0, 9, 8]           # slot 0 takes the back each time
    assert sample_indices([q(0.95), q(0.5), q(0.99)], 10) == [9, 4, 7]
    assert random_int(2147483647, 0, 9) == 9 and random_int(0, 0, 0) == 0
    rng = np.random.default_rng(3)
    for _ in range(200):
        N = int(rng.integers(3, 50))
        idx = sample_indices(rng.integers(0, 2 ** 31, 3), N)
        assert len(set(idx)) == 3 and all(0 <= i < N for i in idx)


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libmatcher_ref.so")), reason="oracle/_ref not built")
def test_random_int_against_the_references_dutils():
    ref = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libmatcher_ref.so"))
    f = getattr(ref, "_ZN6DUtils6Random9RandomIntEii")
    f.restype = ctypes.c_int
    libc = ctypes.CDLL(None)
    for seed in (1, 77, 4242):
        for d in (3, 7, 24, 1000):
            libc.srand(seed)
            got = [f(0, d - 1) for _ in range(50)]
            libc.srand(seed)
            assert got == [random_int(libc.rand(), 0, d - 1) for _ in range(50)]


def test_schedule_against_the_literal_round_robin(tmp_path):
    exe = tmp_path / "sim3_schedule_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "ccm_slam_amd", "host"), "-o", str(exe),
                    os.path.join(HERE, "host", "sim3_schedule_check.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True).stdout
    assert out.startswith("sim3 schedule ok: 200 seeds"), out


def test_kernel_lines_on_the_host_match_the_checker(tmp_path):
    """sim3_ransac_math.h (the kernel's arithmetic) compiled with g++ against the numpy checker: bit-identical (both use glibc's atan2 / sin / cos)."""
    from ccm_slam_amd import sim3, synth
    exe = tmp_path / "sim3_hyp_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe),
                    os.path.join(HERE, "host", "sim3_hyp_check.cpp"), "-lm"], check=True)
    for fix in (0, 1):
        cands = [sim3.Sim3Candidate(**d) for d in synth.make_sim3_candidates(60 + fix, 2, 2, [3, 7, 64, 200], 0.3, bool(fix))]
        cands[2].X1[5] = cands[2].X1[4]; cands[2].X2[5] = cands[2].X2[4]
        rng = np.random.default_rng(fix)
        hc, hi = [], []
        for h in range(120):
            c = int(rng.integers(0, 4))
            hc.append(c); hi.append(rng.choice(cands[c].N, 3, replace=False))
        hc.append(2); hi.append(np.array([4, 5, 6]))                                  # two duplicated points
        hc.append(2); hi.append(np.array([4, 5, 1]))
        pt_off, X1, X2, K1, K2, t1, t2, _, _ = sim3.pack(cands)
        hc = np.array(hc, np.int32); hi = np.array(hi, np.int32)
        with open(tmp_path / "in.bin", "wb") as f:
            f.write(np.array([len(cands), pt_off[-1], len(hc), fix], np.int32).tobytes())
            for a in (pt_off, X1, X2, K1, K2, t1, t2, hc, hi):
                f.write(a.tobytes())
        subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
        raw = (tmp_path / "out.bin").read_bytes()
        o = 0
        for h in range(len(hc)):
            N = cands[hc[h]].N
            n = int(np.frombuffer(raw, np.int32, 1, o)[0]); rts = np.frombuffer(raw, np.float32, 13, o + 4)
            inl = np.frombuffer(raw, np.uint8, N, o + 56).astype(bool); o += 56 + N
            ni, ref, rinl = ref_hypothesis(cands[hc[h]], hi[h], bool(fix))
            want = np.concatenate([ref["R"].reshape(-1), ref["t"], [ref["s"]]]).astype(np.float32)
            assert n == ni and np.array_equal(inl, rinl), h
            assert np.array_equal(rts.view(np.uint32), want.view(np.uint32)) or np.array_equal(rts, want, equal_nan=True), (h, rts, want)


def test_literal_loop_stops_at_the_accepted_event():
    """The checker's ComputeSim3 loop: a true candidate among false ones is found; rejecting events makes the loop go on."""
    from ccm_slam_amd import sim3, synth
    cands = [sim3.Sim3Candidate(**d) for d in synth.make_sim3_candidates(70, 1, 2, [25, 20, 18], 0.2)]
    rng = np.random.default_rng(70)
    draws = rng.integers(0, 2 ** 31, 20000)
    ev = ref_compute_sim3(cands, ArrayDraw(draws), max_iterations=100)
    assert len(ev) == 1 and ev[0][0] == 0 and ev[0][5] > 6
    ev3 = ref_compute_sim3(cands, ArrayDraw(draws), accept=lambda k, e: k >= 2, max_iterations=100)
    assert ev3[0][0] == 0 and len(ev3) >= 2


@pytest.mark.skipif(not os.path.isdir("/root/reference/cslam"), reason="the reference's headers are not present")
def test_sim3solver_translation_unit_against_the_references_real_headers():
    """shim/Sim3Solver_hip.cpp compiled to an object against the reference's REAL Sim3Solver.h / KeyFrame.h / MapPoint.h (make -C shim check_real):
    it defines every cslam::Sim3Solver member that Sim3Solver.cpp defines, leaves undefined only members of the reference's own classes, and
    its iterate() goes to the host library's single-solver entry (one device launch per call)."""
    import re
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "shim"), "-s", "check_real"])
    out = subprocess.run(["nm", "-C", os.path.join(ROOT, "shim", "_real", "Sim3Solver_hip.o")], capture_output=True, text=True, check=True).stdout
    defined = [l.split(" ", 2)[2] for l in out.splitlines() if len(l.split(" ", 2)) == 3 and l.split(" ", 2)[1] in "TW"]
    undefined = [l.strip()[2:] for l in out.splitlines() if l.strip().startswith("U ")]
    for m in ("Sim3Solver(", "SetRansacParameters(", "find(", "iterate(", "GetEstimatedRotation(", "GetEstimatedTranslation(", "GetEstimatedScale(",
              "ComputeCentroid(", "ComputeSim3(", "CheckInliers(", "Project(", "FromCameraToImage("):
        assert any(d.startswith("cslam::Sim3Solver::" + m) for d in defined), m
    foreign = [u for u in undefined if "cslam::" in u.split("(")[0] and not re.match(r"(.* )?cslam::(KeyFrame|MapPoint|Map|Frame)::", u)]
    assert not foreign, foreign
    assert any(u.startswith("ccmh_sim3_solver_iterate") for u in undefined)
