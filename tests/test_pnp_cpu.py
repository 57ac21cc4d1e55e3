"""CPU side of the PnP RANSAC (csrc/pnp_math.h, host/pnp_schedule.h, cslam::PnPRansacBatch with the host evaluator).

Known answers of the restated f64 C-API calls; the restated SVDs against numpy.linalg.svd; a literal Python replay of cslam/src/PnPSolver.cpp (tests/pnp_cases.py)
against the header through libccm_host.so, bit for bit; the strict threshold of CheckInliers; the batched schedule against the sequential solver on supplied draws,
with the FIFO handed to a following Sim3 batch; a noise-free scene; tests/host/pnp_check.cpp under the address and undefined-behaviour sanitizers.

The SVD bounds are measured, not derived: over the sweep of test_restated_svds_against_numpy (40 seeds x n in {4, 5, 12, 40}, half a pixel of noise) the maxima, rounded up to one decimal, were
  singular values, in units of 2^-53 sigma_1:            12x12 M'M 16.2    3x3 (PW0'PW0 and CC) 8.4
  singular vectors, in units of 2^-53 sigma_1 / gap:     12x12 M'M  1.0    3x3                 18.4
and the test asserts 4x of each (other seeds, numpy's other summation order), the margin tests/test_twoview_cpu.py uses.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pnp_cases as pc
from ccm_slam_amd import pnp, sim3
from ccm_slam_amd._lib import CcmError, _p

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U = 2.0 ** -53
C_S12, C_V12, C_S3, C_V3 = 16.2, 1.0, 8.4, 18.4   # measured maxima (module docstring)


def _prim(which, A, b=None, rows=0, n_out=0):
    out = np.zeros(n_out)
    A = np.ascontiguousarray(A, np.float64)
    b = None if b is None else np.ascontiguousarray(b, np.float64)
    rc = pnp._host().ccmh_pnp_primitive(which, rows, _p(A), _p(b), _p(out))
    assert rc >= 0, rc
    return out, rc


def _svd_ut(A):
    n = np.asarray(A).shape[0]
    out, _ = _prim(0 if n == 3 else 1, A, n_out=n + n * n)
    return out[:n], out[n:].reshape(n, n)


# ---- known answers of the restated primitives --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 12])
def test_svd_of_diagonal_and_permuted_diagonal_matrices(n):
    d = np.arange(n, 0, -1.0)                       # already descending: nothing rotates, nothing is swapped
    w, ut = _svd_ut(np.diag(d))
    assert np.array_equal(w, d) and np.array_equal(ut, np.eye(n))
    p = np.random.default_rng(n).permutation(n)     # diag entries in another order: the sort swaps rows, the values stay exact
    w, ut = _svd_ut(np.diag(d[p]))
    assert np.array_equal(w, d)
    want = np.zeros((n, n)); want[np.arange(n), np.argsort(-d[p], kind="stable")] = 1
    assert np.array_equal(ut, want)


def test_svd_tie_keeps_the_first_index():
    w, ut = _svd_ut(np.diag([2.0, 5.0, 5.0]))
    assert np.array_equal(w, [5.0, 5.0, 2.0])
    # selection sort with a strict <: the first 5 (index 1) is taken first; the swap puts row 0 where it stood, so row 2 (the second 5) comes next
    assert np.array_equal(ut, [[0, 1, 0], [0, 0, 1], [1, 0, 0]])
    out, _ = _prim(2, np.diag([3.0, 3.0, 1.0]), n_out=21)     # cvSVD with U and V
    assert np.array_equal(out[:3], [3.0, 3.0, 1.0]) and np.array_equal(out[3:12].reshape(3, 3), np.eye(3)) and np.array_equal(out[12:].reshape(3, 3), np.eye(3))


def test_cvinvert_svd_of_a_singular_diagonal_is_the_pseudo_inverse():
    out, _ = _prim(3, np.diag([2.0, 1.0, 0.0]), n_out=9)
    assert np.array_equal(out.reshape(3, 3), np.diag([0.5, 1.0, 0.0]))
    out, _ = _prim(3, np.diag([4.0, 2.0, 8.0]), n_out=9)
    assert np.array_equal(out.reshape(3, 3), np.diag([0.25, 0.5, 0.125]))


def test_cvsolve_svd_small_integer_system():
    # orthogonal columns with norms 2, 2, 2, 2 (a 6x4 with small-integer entries): the Jacobi sweep finds nothing to rotate and every step is exact
    A = np.array([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1], [0, 0, 0, 0], [0, 0, 0, 0]], np.float64)
    x = np.array([3.0, -2.0, 5.0, 1.0])
    out, _ = _prim(5, A, A @ x, n_out=4)
    assert np.array_equal(out, x)
    A3 = np.array([[2, 0, 0], [0, 4, 0], [0, 0, 8], [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float64)
    out, _ = _prim(4, A3, A3 @ np.array([1.0, -3.0, 2.0]), n_out=3)
    assert np.array_equal(out, [1.0, -3.0, 2.0])
    A5 = np.zeros((6, 5)); A5[np.arange(5), np.arange(5)] = [16, 8, 4, 2, 1]
    out, _ = _prim(6, A5, A5 @ np.array([1.0, 2.0, 3.0, 4.0, 5.0]), n_out=5)
    assert np.array_equal(out, [1.0, 2.0, 3.0, 4.0, 5.0])


@pytest.mark.parametrize("cols,which", [(3, 7), (12, 8)])
def test_cvmultransposed_is_exact_and_symmetric_on_integers(cols, which):
    A = np.random.default_rng(cols).integers(-9, 10, (7, cols)).astype(np.float64)
    out, _ = _prim(which, A, rows=7, n_out=cols * cols)
    D = out.reshape(cols, cols)
    assert np.array_equal(D, A.T @ A) and np.array_equal(D, D.T)


def test_qr_solve_exact_answer_and_singular_exit():
    A = np.array([[2, 0, 0, 0], [0, 4, 0, 0], [0, 0, 8, 0], [0, 0, 0, 16], [0, 0, 0, 0], [0, 0, 0, 0]], np.float64)
    x = np.array([1.0, -2.0, 0.5, 3.0])
    out = np.full(4, 7.0)
    assert pnp._host().ccmh_pnp_primitive(9, 0, _p(A), _p(A @ x), _p(out)) == 1
    assert np.array_equal(out, x)
    # a zero column: the reference prints and returns with X untouched
    A[:, 2] = 0
    out = np.array([7.0, -7.0, 7.5, 0.25])
    assert pnp._host().ccmh_pnp_primitive(9, 0, _p(A), _p(A @ x), _p(out)) == 0
    assert np.array_equal(out, [7.0, -7.0, 7.5, 0.25])


# ---- the restated SVDs against numpy -------------------------------------------------------------------------------------------------------------------
def _matrices(c, n):
    pws, us = pc.gather(c, range(n))
    pws = np.ascontiguousarray(pws); us = np.ascontiguousarray(us); cam = np.ascontiguousarray(c.cam, np.float64)
    mtm = np.zeros(144); pca = np.zeros(9); cc = np.zeros(9)
    assert pnp._host().ccmh_pnp_matrices(n, _p(pws), _p(us), _p(cam), _p(mtm), _p(pca), _p(cc)) == 0
    return mtm.reshape(12, 12), pca.reshape(3, 3), cc.reshape(3, 3)


def _against_numpy(A, rows):
    w, ut = _svd_ut(A)
    u, s, _ = np.linalg.svd(A)
    cs = np.abs(w - s).max() / (U * s[0])
    cv = 0.0
    for i in rows:
        gap = min(abs(s[i] - s[j]) for j in range(len(s)) if j != i)
        d = min(np.abs(ut[i] - u[:, i]).max(), np.abs(ut[i] + u[:, i]).max())
        cv = max(cv, d / (U * s[0] / gap))
    return cs, cv


def test_restated_svds_against_numpy():
    """The 12x12 M'M and the two 3x3 matrices (PW0'PW0, CC) of real compute_pose calls.  The four trailing rows of M'M's Ut are compared where they are determined:
    n >= 12 correspondences with half a pixel of noise (with n = 4 or 5 the null space of M has more than one dimension)."""
    m = dict(s12=0.0, v12=0.0, s3=0.0, v3=0.0)
    for seed in range(40):
        for n in (4, 5, 12, 40):
            c = pc.make_candidate(1000 + seed, n)
            c.P2D = (np.asarray(c.P2D) + np.random.default_rng(seed).normal(0, 0.5, (n, 2))).astype(np.float32)
            mtm, pca, cc = _matrices(c, n)
            cs, cv = _against_numpy(mtm, range(8, 12) if n >= 12 else [])
            m["s12"] = max(m["s12"], cs); m["v12"] = max(m["v12"], cv)
            for A in (pca, cc):
                cs, cv = _against_numpy(A, range(3))
                m["s3"] = max(m["s3"], cs); m["v3"] = max(m["v3"], cv)
    print("restated f64 SVDs against numpy, measured maxima:", {k: round(v, 2) for k, v in m.items()})
    assert m["s12"] <= 4 * C_S12 and m["v12"] <= 4 * C_V12 and m["s3"] <= 4 * C_S3 and m["v3"] <= 4 * C_V3, m


# ---- the literal replay against the header ---------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("n", [4, 5, 12, 40])
def test_compute_pose_check_inliers_and_refine_equal_the_literal_replay_bit_for_bit(n):
    for seed in range(6):
        c = pc.make_candidate(200 + 10 * n + seed, n, n_out=n // 2, cam=(480.0 + seed, 470.0, 310.0, 250.0 - seed), sigma2=1.0 + 0.2 * seed)
        idx = np.nonzero(c.meta["true"])[0] if seed % 2 else np.arange(n)      # exact samples, and samples with outliers among them
        pws, us = pc.gather(c, idx)
        R, t, rep, N = pc.compute_pose(pws, us, c.cam)
        R2, t2, rep2, N2 = pnp.compute_pose(pws, us, c.cam)
        assert N == N2 and np.array_equal(_bits(R), _bits(R2)) and np.array_equal(_bits(t), _bits(t2)) and np.array_equal(_bits(rep), _bits(rep2)), (n, seed)
        me = pnp.max_errors(c.sigma2)
        k, m, e2 = pc.check_inliers(R, t, c.cam, np.asarray(c.P3Dw).reshape(-1, 3), np.asarray(c.P2D).reshape(-1, 2), me)
        k2, m2, e22 = pnp.check_inliers(c, np.concatenate([R2.reshape(-1), t2]))
        assert k == k2 and np.array_equal(m, m2) and np.array_equal(e2.view(np.uint32), e22.view(np.uint32)), (n, seed)
        # Refine on that mask (at least four inliers): gather, compute_pose, CheckInliers
        if k >= 4:
            ridx = np.nonzero(m)[0]
            rp, ru = pc.gather(c, ridx)
            Rr, tr, _, _ = pc.compute_pose(rp, ru, c.cam)
            kr, mr, _ = pc.check_inliers(Rr, tr, c.cam, np.asarray(c.P3Dw).reshape(-1, 3), np.asarray(c.P2D).reshape(-1, 2), me)
            kr2, mr2, Rt = pnp.refine(c, m)
            assert kr == kr2 and np.array_equal(mr, mr2) and np.array_equal(_bits(np.concatenate([np.reshape(Rr, -1), tr])), _bits(Rt)), (n, seed)


def test_four_point_hypotheses_of_the_evaluator_equal_the_literal_replay():
    c = pc.make_candidate(31, 30, 10)
    rng = np.random.default_rng(31)
    hi = np.array([rng.choice(c.N, 4, replace=False) for _ in range(12)])
    n_inl, Rt, masks = pnp.eval_hypotheses_host([c], np.zeros(12, np.int32), hi)
    for h in range(12):
        pws, us = pc.gather(c, hi[h])
        R, t, _, _ = pc.compute_pose(pws, us, c.cam)
        assert np.array_equal(_bits(np.concatenate([np.reshape(R, -1), t])), _bits(Rt[h])), h
        k, m, _ = pc.check_inliers(R, t, c.cam, c.P3Dw, c.P2D, pnp.max_errors(c.sigma2))
        assert k == n_inl[h] and np.array_equal(m, masks[h]), h


# ---- CheckInliers' strict threshold --------------------------------------------------------------------------------------------------------------------------
def threshold_edge_candidates():
    """One candidate, one sample; a point's error2 under that sample's pose becomes its threshold: (candidate with max_err = error2, candidate with
    max_err = nextafter(error2, +inf), the sample, the point).  sigma2 carries the threshold (th2 = 1)."""
    c = pc.make_candidate(77, 20, 6)
    sample = np.nonzero(c.meta["true"])[0][:4]
    n_inl, Rt, _ = pnp.eval_hypotheses_host([c], [0], [sample], th2=1.0)
    _, _, e2 = pnp.check_inliers(c, Rt[0], th2=1.0)
    i = int(np.nonzero(~c.meta["true"])[0][0])
    assert e2[i] > 100
    at, above = [pnp.PnPCandidate(P3Dw=c.P3Dw, P2D=c.P2D, sigma2=np.array(c.sigma2, np.float32), cam=c.cam) for _ in range(2)]
    at.sigma2[i] = e2[i]
    above.sigma2[i] = np.nextafter(e2[i], np.float32(np.inf))
    return at, above, sample, i


def test_threshold_is_strict():
    at, above, sample, i = threshold_edge_candidates()
    _, _, m_at = pnp.eval_hypotheses_host([at], [0], [sample], th2=1.0)
    _, _, m_above = pnp.eval_hypotheses_host([above], [0], [sample], th2=1.0)
    assert not m_at[0][i] and m_above[0][i]
    assert np.array_equal(np.delete(m_at[0], i), np.delete(m_above[0], i))


# ---- the schedule against the sequential solver --------------------------------------------------------------------------------------------------------------
def schedule_fixture():
    """Three candidates: 40 exact correspondences and gross outliers (sigma2 = 1), one with N < mRansacMinInliers, and one whose outliers outnumber the rest."""
    cands = [pc.make_candidate(1, 40, 25, sparse=True), pc.make_candidate(2, 6, 0), pc.make_candidate(3, 40, 40, cam=(450.0, 450.0, 300.0, 200.0))]
    raws = np.random.default_rng(5).integers(0, 2 ** 31 - 1, 4000)
    return cands, raws


def _same_event(got, want):
    i, Tcw, vb, n, refined, no_more = want
    return (got["cand"] == i and got["n_inliers"] == n and got["refined"] == refined and got["no_more"] == no_more and np.array_equal(got["inliers"], vb) and
            np.array_equal(got["Tcw"].view(np.uint32), Tcw.view(np.uint32)))


def test_schedule_equals_the_sequential_solver_on_supplied_draws():
    cands, raws = schedule_fixture()
    want, solvers, used = pc.sequential_events(cands, raws)
    # what the fixture must show, on the replay itself
    assert any(e[4] for e in want), "no refined pose"
    assert solvers[1].N < solvers[1].mRansacMinInliers and solvers[1].mnIterations == 0, "no candidate discarded before a draw"
    assert sum(s.refine_at_non_best for s in solvers) > 0, "no hypothesis reached the threshold without beating the best"
    assert any(e[5] and not e[4] for e in want), "no call ran out of iterations with a best pose"
    sim3.clear_draws()
    b = pnp.PnPRansac(cands, device=None, draws=raws)
    got = []
    while True:
        r = b.next()
        if r is None:
            break
        got.append(r)
    assert len(got) == len(want) and all(_same_event(g, w) for g, w in zip(got, want))
    assert [b.info(c)[0] for c in range(3)] == [s.mnIterations for s in solvers]
    assert [b.info(c)[1:3] for c in range(3)] == [(s.mRansacMaxIts, s.mRansacMinInliers) for s in solvers]
    src, hyps, passes, refines = b.stats()
    assert src - sim3.draws_pending().size == used          # nothing the sequential solver did not draw is lost: it waits in the FIFO
    assert refines < sum(s.n_refine_calls for s in solvers)  # Refine is computed once per best mask, not once per hypothesis at the threshold
    assert passes <= len(want) + 1
    b.close()
    sim3.clear_draws()


def test_fifo_goes_to_the_next_consumer_of_the_thread():
    """After the first pose, a Sim3 batch on the same thread draws exactly what the sequential reference would have drawn next."""
    from ccm_slam_amd import synth
    cands, raws = schedule_fixture()
    want, _, used = pc.sequential_events(cands, raws, max_events=1)
    sim3.clear_draws()
    b = pnp.PnPRansac(cands, device=None, draws=raws)
    got = b.next()
    assert _same_event(got, want[0])
    pending = sim3.draws_pending()
    src = b.stats()[0]
    assert pending.size > 0 and src == used + pending.size and np.array_equal(pending, raws[used:src])
    # a second PnP batch drinks from the FIFO first: its first pose is the one a sequential solver finds on raws[used:]
    want2, _, used2 = pc.sequential_events(cands[2:], raws[used:], max_events=1)
    b2 = pnp.PnPRansac(cands[2:], device=None, draws=raws[src:])
    assert _same_event(b2.next(), want2[0])
    left = sim3.draws_pending()
    assert np.array_equal(left, raws[used + used2:used + used2 + left.size])
    # and the Sim3 schedule's own check of the same hand-back runs in tests/host/pnp_check.cpp (a Sim3 schedule after every PnP one)
    b.close(); b2.close()
    sim3.clear_draws()


def test_first_iterate_without_success_runs_to_the_iteration_limit():
    """The loop condition is `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`: iterate(5) of a candidate that never succeeds consumes
    4 * max(mRansacMaxIts, 5) draws and returns bNoMore."""
    c = pc.make_candidate(9, 9, 60)     # nine true correspondences among 69: a sample of four true ones is rare
    raws = np.random.default_rng(11).integers(0, 2 ** 31 - 1, 4000)
    for max_its, want_h in ((3, 5), (40, 40)):
        sim3.clear_draws()
        b = pnp.PnPRansac([c], device=None, draws=raws, max_iterations=max_its)
        assert b.info(0)[1] == max_its
        pose, no_more = b.iterate(0, 5)
        s = pc.RefSolver(c, pc.ArrayDraw(raws), maxIterations=max_its)
        Tcw, ref_no_more, _, _ = s.iterate(5)
        assert Tcw is None and pose is None and no_more and ref_no_more
        assert b.stats()[0] == 4 * want_h == s.draw.at and sim3.draws_pending().size == 0
        b.close()


def test_min_set_other_than_four_is_an_error():
    with pytest.raises(CcmError):
        pnp.PnPRansac([pc.make_candidate(1, 12)], device=None, min_set=5)


# ---- a scene without noise ------------------------------------------------------------------------------------------------------------------------------------
def test_noise_free_scene_refined_pose_separates_true_from_gross():
    """40 exact correspondences (rounded to f32) and 25 outliers displaced by 30 to 80 pixels: under the refined pose every true correspondence is an inlier
    (its error is the f32 rounding of the projection, far below mvMaxError = 5.991) and no gross outlier is."""
    c = pc.make_candidate(1, 40, 25, sparse=True)
    b = pnp.PnPRansac([c], device=None, draws=np.random.default_rng(5).integers(0, 2 ** 31 - 1, 4000))
    r = b.next()
    assert r is not None and r["refined"] and r["n_inliers"] == 40
    want = np.zeros(c.n_matches, bool); want[c.kp_idx[c.meta["true"]]] = True
    assert np.array_equal(r["inliers"], want)
    assert np.abs(r["Tcw"][:3, :3] - c.meta["R"]).max() < 1e-4 and np.abs(r["Tcw"][:3, 3] - c.meta["t"]).max() < 1e-3
    assert np.array_equal(r["Tcw"][3], [0, 0, 0, 1])
    b.close()
    sim3.clear_draws()


# ---- the stand-alone program under the sanitizers ------------------------------------------------------------------------------------------------------------
def test_schedule_and_header_under_the_sanitizers(tmp_path):
    exe = tmp_path / "pnp_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "ccm_slam_amd", "host"), "-o", str(exe), os.path.join(HERE, "host", "pnp_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and re.search(r"pnp schedule ok: \d+ seeds, \d+ events, \d+ hypotheses", r.stdout) and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.skipif(not os.path.isdir("/root/reference/cslam"), reason="the reference's headers are not present")
def test_pnpsolver_translation_unit_against_the_references_real_header():
    """shim/PnPsolver_hip.cpp compiled to an object against the reference's REAL PnPSolver.h (make -C shim check_real): it defines the constructor,
    SetRansacParameters, find and iterate, leaves the private EPnP members undefined, and goes to the host library's batch."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "shim"), "-s", "check_real"])
    out = subprocess.run(["nm", "-C", os.path.join(ROOT, "shim", "_real", "PnPsolver_hip.o")], capture_output=True, text=True, check=True).stdout
    defined = [l.split(" ", 2)[2] for l in out.splitlines() if len(l.split(" ", 2)) == 3 and l.split(" ", 2)[1] in "TW"]
    undefined = [l.strip()[2:] for l in out.splitlines() if l.strip().startswith("U ")]
    for m in ("PnPsolver(", "~PnPsolver(", "SetRansacParameters(", "find(", "iterate("):
        assert any(d.startswith("cslam::PnPsolver::" + m) for d in defined), m
    for m in ("compute_pose(", "CheckInliers(", "Refine(", "qr_solve("):
        assert not any(d.startswith("cslam::PnPsolver::" + m) for d in defined), m
    foreign = [u for u in undefined if "cslam::" in u.split("(")[0] and not re.match(r"(.* )?cslam::(KeyFrame|MapPoint|Map|Frame)::", u)]
    assert not foreign, foreign
    assert any(u.startswith("ccmh_pnp_ransac_iterate") for u in undefined)
