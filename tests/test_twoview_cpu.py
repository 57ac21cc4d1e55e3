"""CPU: the two-view initialiser's arithmetic (ccm_slam_amd/csrc/twoview_math.h compiled with g++ into libccm_host.so).

Known answers for the restated cv::SVDecomp (3x3, 16x9, 8x9, the completion of rows without a singular value); numpy.linalg.svd in f64 on the same f32
matrices as the yardstick; an independent numpy-f32 replay of Normalize, CheckHomography, CheckFundamental and one CheckRT match (bit-identical scores, masks,
statuses and points); cslam::TwoViewInitializer through its host evaluator against a literal sequential replay of FindHomography / FindFundamental / CheckRT;
and the H / F branch on the planar and the general scene."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_triangulate_cpu import jacobi_svd4, same_bits

f32, f64 = np.float32, np.float64
EPS24 = 2.0 ** -24

# The restated decompositions against numpy.linalg.svd in f64 on the same f32 matrices, over the seeded sweep of sweep_matrices() (the 16x9, 8x9 and 3x3
# matrices of 4 scenes x 3 sizes x 40 sets = 480 of each shape).  Units: the null vector (up to sign) in 2^-24 * sigma1 / gap, gap = the distance of its
# singular value to the neighbouring one (sigma8 - sigma9 for 16x9, sigma8 for the rank-8 8x9); the 3x3 singular values in 2^-24 * sigma1; the rank-2 product
# u diag(w1, w2, 0) vt = A - sigma3 u3 v3' in 2^-24 * sigma1 * (1 + sigma3 / (sigma2 - sigma3)): u3 and v3 move by eps * sigma1 / (sigma2 - sigma3).
# Measured maxima (measure_c()); asserted at 4 x them: the margin covers other seeds and another summation order.
C_H = 1.476       # 16x9 null vector
C_F = 0.399       # 8x9 completed row
C_W3 = 4.225      # 3x3 singular values
C_RANK2 = 5.035   # 3x3 rank-2 product
C_MARGIN = 4.0


def tv():
    from ccm_slam_amd import twoview
    return twoview


# ---------------------------------------------------------------------------------------------------------------------------------------------
# known answers of the restated SVD
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_diagonal_and_permuted_diagonal_3x3():
    w, u, vt = tv().svd(np.diag([3, 2, 1]).astype(f32))
    assert np.array_equal(w, [3, 2, 1]) and np.array_equal(u, np.eye(3)) and np.array_equal(vt, np.eye(3))
    A = np.zeros((3, 3), f32); A[0, 1] = 2; A[1, 2] = 5; A[2, 0] = 1
    w, u, vt = tv().svd(A)
    assert np.array_equal(w, [5, 2, 1])
    assert np.array_equal(u, [[0, 1, 0], [1, 0, 0], [0, 0, 1]]) and np.array_equal(vt, [[0, 0, 1], [0, 1, 0], [1, 0, 0]])
    assert np.array_equal((u * w) @ vt, A)


def test_a_tie_keeps_the_first_index():
    w, u, vt = tv().svd(np.diag([2, 2, 1]).astype(f32))
    assert np.array_equal(w, [2, 2, 1]) and np.array_equal(vt, np.eye(3)) and np.array_equal(u, np.eye(3))
    w, u, vt = tv().svd(np.diag([1, 2, 2]).astype(f32))          # the first 2 (index 1) is moved to the front, then the second
    assert np.array_equal(w, [2, 2, 1]) and np.array_equal(vt, [[0, 1, 0], [0, 0, 1], [1, 0, 0]])


def test_rank_8_16x9_matrix_with_a_closed_form_null_vector():
    # every row is orthogonal to n = (1, -2, 2, 0, 4, -4, 0, 2, 6) / 9 by construction with small integers: the products are exact in f32
    n = np.array([1, -2, 2, 0, 4, -4, 0, 2, 6], f64)
    assert n @ n == 81
    rng = np.random.default_rng(3)
    A = np.zeros((16, 9), f32)
    for r in range(16):
        while True:
            a = rng.integers(-4, 5, 9).astype(f64)
            k = int(rng.integers(0, 9))
            if n[k] == 0:
                continue
            a[k] = 0
            rest = a @ n
            if rest % n[k] == 0:
                a[k] = -rest / n[k]
                break
        assert a @ n == 0
        A[r] = a
    assert np.linalg.matrix_rank(A.astype(f64)) == 8
    v = tv().svd(A)
    s = np.linalg.svd(A.astype(f64), compute_uv=False)
    err = min(np.abs(v - n / 9).max(), np.abs(v + n / 9).max())
    assert err <= 4 * C_H * EPS24 * s[0] / s[7], err


def test_8x9_completed_row_is_orthogonal_to_the_eight_input_rows():
    rng = np.random.default_rng(5)
    for _ in range(20):
        A = rng.normal(0, 1, (8, 9)).astype(f32)
        vt = tv().svd(A)
        s = np.linalg.svd(A.astype(f64), compute_uv=False)
        assert np.abs(A.astype(f64) @ vt[8].astype(f64)).max() <= 64 * EPS24 * s[0]
        assert abs(np.linalg.norm(vt[8].astype(f64)) - 1) <= 8 * EPS24
        assert np.abs(vt.astype(f64) @ vt.astype(f64).T - np.eye(9)).max() <= 64 * EPS24 * s[0] / s[7]


def test_two_zero_rows_run_the_completion_below_n():
    A = np.zeros((3, 3), f32); A[0] = [1, 2, 3]                  # At has the rows (1 0 0), (2 0 0), (3 0 0): two singular values are 0
    w, u, vt = tv().svd(A)
    assert abs(float(w[0]) - np.sqrt(14.0)) <= 4 * EPS24 * np.sqrt(14.0) and w[1] == 0 and w[2] == 0   # the rotations round in f32
    assert np.abs(u.astype(f64).T @ u.astype(f64) - np.eye(3)).max() <= 8 * EPS24    # the completed columns of u are orthonormal
    assert np.abs(np.abs(u[:, 0]) - [1, 0, 0]).max() <= 4 * EPS24
    # the completion starts from +-1/3 vectors of cv::RNG(0x12345678): the first completed row is fixed by the first three draws
    state = 0x12345678
    signs = []
    for _ in range(3):
        state = ((state & 0xffffffff) * 4164903690 + (state >> 32)) & 0xffffffffffffffff
        signs.append(1.0 if (state & 0xffffffff) & 256 else -1.0)
    r = np.array(signs) / 3
    r -= (r @ u[:, 0].astype(f64)) * u[:, 0].astype(f64)
    r /= np.linalg.norm(r)
    assert np.abs(u[:, 1] - r).max() <= 8 * EPS24
    # an 8x9 matrix with two zero rows: the completion runs for rows below n and for the ninth row
    rng = np.random.default_rng(9)
    A = rng.normal(0, 1, (8, 9)).astype(f32); A[2] = 0; A[6] = 0
    vt = tv().svd(A)
    assert np.abs(vt.astype(f64) @ vt.astype(f64).T - np.eye(9)).max() <= 64 * EPS24
    assert np.abs(A.astype(f64) @ vt[6:].astype(f64).T).max() <= 64 * EPS24 * np.linalg.norm(A.astype(f64), 2)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the yardstick: numpy.linalg.svd in f64
# ---------------------------------------------------------------------------------------------------------------------------------------------
def build_A(p1, p2):
    """The matrices of ComputeH21 (16, 9) and ComputeF21 (8, 9) for eight normalised points, in f32"""
    u1, v1, u2, v2 = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    z, o = np.zeros(8, f32), np.ones(8, f32)
    AH = np.zeros((16, 9), f32)
    AH[0::2] = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], 1)
    AH[1::2] = np.stack([u1, v1, o, z, z, z, (-u2) * u1, (-u2) * v1, -u2], 1)
    AF = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, o], 1).astype(f32)
    return AH, AF


def sweep_matrices():
    out = []
    for kind, seed in (("planar", 11), ("general", 12), ("planar", 13), ("general", 14)):
        for N in (8, 64, 300):
            sc = tv().make_scene(kind, N, seed=seed, unmatched=N // 3, outliers=0.1)
            a = tv().ransac_inputs(sc)
            for s in tv().random_sets(N, 40, seed):
                out.append(build_A(a[2][s], a[3][s]))
    return out


def _sign_err(v, ref):
    return min(np.abs(v - ref).max(), np.abs(v + ref).max())


def measure_c():
    cH = cF = cW = cR = 0.0
    for AH, AF in sweep_matrices():
        _, s, vt = np.linalg.svd(AH.astype(f64))
        cH = max(cH, _sign_err(tv().svd(AH).astype(f64), vt[8]) / (EPS24 * s[0] / (s[7] - s[8])))
        _, s, vt = np.linalg.svd(AF.astype(f64))
        mine = tv().svd(AF)[8]
        cF = max(cF, _sign_err(mine.astype(f64), vt[8]) / (EPS24 * s[0] / s[7]))
        Fpre = mine.reshape(3, 3)
        w, u, vt3 = tv().svd(Fpre)
        U, s, Vt = np.linalg.svd(Fpre.astype(f64))
        cW = max(cW, np.abs(w.astype(f64) - s).max() / (EPS24 * s[0]))
        rank2 = (u.astype(f64) * np.array([w[0], w[1], 0.0])) @ vt3.astype(f64)
        ref2 = (U * np.array([s[0], s[1], 0.0])) @ Vt
        cR = max(cR, np.abs(rank2 - ref2).max() / (EPS24 * s[0] * (1 + s[2] / (s[1] - s[2]))))
    return cH, cF, cW, cR


def test_restated_svd_against_numpy_f64():
    cH, cF, cW, cR = measure_c()
    print(f"16x9 null vector c = {cH:.3f}, 8x9 completed row c = {cF:.3f}, 3x3 singular values c = {cW:.3f}, rank-2 product c = {cR:.3f}")
    assert cH <= C_MARGIN * C_H and cF <= C_MARGIN * C_F and cW <= C_MARGIN * C_W3 and cR <= C_MARGIN * C_RANK2


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the checker: an independent numpy-f32 replay
# ---------------------------------------------------------------------------------------------------------------------------------------------
def ref_normalize(xy):
    xy = np.asarray(xy, f32)
    n = len(xy)
    mean = np.add.accumulate(xy, axis=0, dtype=f32)[-1] / f32(n)          # accumulate runs left to right
    d = (xy - mean).astype(f32)
    dev = np.add.accumulate(np.abs(d), axis=0, dtype=f32)[-1] / f32(n)
    s = (1.0 / dev.astype(f64)).astype(f32)
    T = np.eye(3, dtype=f32)
    T[0, 0] = s[0]; T[1, 1] = s[1]; T[0, 2] = -mean[0] * s[0]; T[1, 2] = -mean[1] * s[1]
    return (d * s).astype(f32), T


def ref_inv33(S):
    S = np.asarray(S, f32).reshape(3, 3).astype(f64)
    cof = lambda a, b, c, d: S[a] * S[b] - S[c] * S[d]
    det = S[0, 0] * cof((1, 1), (2, 2), (1, 2), (2, 1)) - S[0, 1] * cof((1, 0), (2, 2), (1, 2), (2, 0)) + S[0, 2] * cof((1, 0), (2, 1), (1, 1), (2, 0))
    if det == 0:
        return np.zeros((3, 3), f32)
    d = 1.0 / det
    t = [cof((1, 1), (2, 2), (1, 2), (2, 1)), cof((0, 2), (2, 1), (0, 1), (2, 2)), cof((0, 1), (1, 2), (0, 2), (1, 1)),
         cof((1, 2), (2, 0), (1, 0), (2, 2)), cof((0, 0), (2, 2), (0, 2), (2, 0)), cof((0, 2), (1, 0), (0, 0), (1, 2)),
         cof((1, 0), (2, 1), (1, 1), (2, 0)), cof((0, 1), (2, 0), (0, 0), (2, 1)), cof((0, 0), (1, 1), (0, 1), (1, 0))]
    return (np.array(t) * d).astype(f32).reshape(3, 3)


def _score(terms):
    """the sequential f32 sum of the interleaved terms; a skipped term adds +0, which changes nothing"""
    return np.add.accumulate(np.concatenate([[f32(0)], terms.reshape(-1)]).astype(f32), dtype=f32)[-1]


def ref_check_h(H21, xy1, xy2, sigma):
    """CheckHomography: (score, inlier flags)"""
    h = np.asarray(H21, f32).reshape(-1); hi = ref_inv33(H21).reshape(-1)
    u1, v1, u2, v2 = xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1]
    inv = f32(1.0 / f64(f32(sigma) * f32(sigma)))
    th = f32(5.991)
    with np.errstate(all="ignore"):
        def side(m, ua, va, ub, vb):
            w = (1.0 / (m[6] * ua + m[7] * va + m[8]).astype(f64)).astype(f32)
            x = (m[0] * ua + m[1] * va + m[2]) * w
            y = (m[3] * ua + m[4] * va + m[5]) * w
            return (((ub - x) * (ub - x) + (vb - y) * (vb - y)) * inv).astype(f32)
        chi1 = side(hi, u2, v2, u1, v1); chi2 = side(h, u1, v1, u2, v2)
        out1, out2 = chi1 > th, chi2 > th
        terms = np.stack([np.where(out1, f32(0), th - chi1), np.where(out2, f32(0), th - chi2)], 1).astype(f32)
    return _score(terms), ~(out1 | out2)


def ref_check_f(F21, xy1, xy2, sigma):
    f = np.asarray(F21, f32).reshape(-1)
    u1, v1, u2, v2 = xy1[:, 0], xy1[:, 1], xy2[:, 0], xy2[:, 1]
    inv = f32(1.0 / f64(f32(sigma) * f32(sigma)))
    th, thScore = f32(3.841), f32(5.991)
    with np.errstate(all="ignore"):
        a2 = f[0] * u1 + f[1] * v1 + f[2]; b2 = f[3] * u1 + f[4] * v1 + f[5]; c2 = f[6] * u1 + f[7] * v1 + f[8]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = ((num2 * num2 / (a2 * a2 + b2 * b2)) * inv).astype(f32)
        a1 = f[0] * u2 + f[3] * v2 + f[6]; b1 = f[1] * u2 + f[4] * v2 + f[7]; c1 = f[2] * u2 + f[5] * v2 + f[8]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = ((num1 * num1 / (a1 * a1 + b1 * b1)) * inv).astype(f32)
        out1, out2 = chi1 > th, chi2 > th
        terms = np.stack([np.where(out1, f32(0), thScore - chi1), np.where(out2, f32(0), thScore - chi2)], 1).astype(f32)
    return _score(terms), ~(out1 | out2)


def ref_prepare_rt(K, R, t):
    K = np.asarray(K, f32).reshape(3, 3); R = np.asarray(R, f32).reshape(3, 3); t = np.asarray(t, f32).reshape(3)
    Rt = np.concatenate([R, t[:, None]], 1)
    P2 = ((K[:, 0:1] * Rt[0:1] + K[:, 1:2] * Rt[1:2]).astype(f32) + K[:, 2:3] * Rt[2:3]).astype(f32)
    P2 = (P2.astype(f64) * 1.0 + 0.0).astype(f32)                        # (float)(t * alpha + 0 * beta): a -0 becomes +0
    O2 = np.zeros(3, f64)
    for k in range(3):
        O2 = O2 + R[k].astype(f64) * f64(t[k])
    return np.concatenate([P2.reshape(-1), (O2 * -1.0 + 0.0).astype(f32), R.reshape(-1), t])


def ref_check_rt(rec, K, xy1, xy2, inliers, th2):
    """One hypothesis: (status (N,), x3d (N, 3), cosParallax (N,)) with NaN where the match is no inlier"""
    rec = np.asarray(rec, f32); K = np.asarray(K, f32).reshape(3, 3)
    P2 = rec[:12].reshape(3, 4); O2 = rec[12:15]; R = rec[15:24].reshape(3, 3); t = rec[24:27]
    P1 = np.concatenate([K, np.zeros((3, 1), f32)], 1)
    N = len(xy1)
    x1, y1, x2, y2 = (xy1[:, 0:1], xy1[:, 1:2], xy2[:, 0:1], xy2[:, 1:2])
    th2 = f32(th2)
    with np.errstate(all="ignore"):
        A = np.stack([x1 * P1[2] - P1[0], y1 * P1[2] - P1[1], x2 * P2[2] - P2[0], y2 * P2[2] - P2[1]], 1).astype(f32)
        _, vt = jacobi_svd4(A)
        v = vt[:, 3, :]
        inv = (1.0 / v[:, 3].astype(f64)).astype(f32)
        X = (v[:, :3] * inv[:, None] + f32(0)).astype(f32)
        finite = np.isfinite(X).all(1)
        n1 = X.copy(); n2 = (X - O2).astype(f32)
        nrm = lambda D: np.sqrt(((D[:, 0].astype(f64) ** 2 + D[:, 1].astype(f64) ** 2) + D[:, 2].astype(f64) ** 2)).astype(f32)
        d1, d2 = nrm(n1), nrm(n2)
        dot = (n1[:, 0].astype(f64) * n2[:, 0] + n1[:, 1].astype(f64) * n2[:, 1]) + n1[:, 2].astype(f64) * n2[:, 2]
        cosp = (dot / (d1 * d2).astype(f64)).astype(f32)
        low = ~(cosp.astype(f64) < 0.99998)
        X2 = np.stack([(((R[r, 0] * X[:, 0] + R[r, 1] * X[:, 1]).astype(f32) + R[r, 2] * X[:, 2]).astype(f64) + f64(t[r])).astype(f32) for r in range(3)], 1)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        def err(Xc, px, py):
            iz = (1.0 / Xc[:, 2].astype(f64)).astype(f32)
            u = fx * Xc[:, 0] * iz + cx; w = fy * Xc[:, 1] * iz + cy
            return ((u - px) * (u - px) + (w - py) * (w - py)).astype(f32)
        e1, e2 = err(X, x1[:, 0], y1[:, 0]), err(X2, x2[:, 0], y2[:, 0])
    st = np.where(low, 6, 7)
    for code, gate in ((5, e2 > th2), (4, e1 > th2), (3, (X2[:, 2] <= 0) & ~low), (2, (X[:, 2] <= 0) & ~low), (1, ~finite)):
        st = np.where(gate, code, st)                                    # the earliest gate is applied last, so it wins
    cosp = np.where(st == 1, f32(np.nan), cosp)
    inl = np.asarray(inliers, bool)
    st = np.where(inl, st, 0)
    X = np.where(inl[:, None], X, f32(np.nan)); cosp = np.where(inl, cosp, f32(np.nan))
    return st.astype(np.uint8), X.astype(f32), cosp.astype(f32)


def scenes_for_the_checker():
    """scenes with unmatched keypoints and outliers, one with NaN / Inf keypoints"""
    out = []
    for kind, N, seed in (("planar", 64, 21), ("general", 65, 22), ("general", 300, 23), ("planar", 9, 24), ("general", 8, 25)):
        out.append(tv().make_scene(kind, N, seed=seed, unmatched=N // 4, outliers=0.15))
    sc = tv().make_scene("general", 40, seed=26, outliers=0.1)
    sc["xy1"] = sc["xy1"].copy(); sc["xy2"] = sc["xy2"].copy()
    sc["xy1"][3, 0] = np.nan; sc["xy2"][7, 1] = np.inf; sc["xy1"][11] = -np.inf; sc["xy2"][12] = np.nan
    out.append(sc)
    return out


def test_normalize_and_inverse_on_the_host_match_the_checker():
    for sc in scenes_for_the_checker():
        for keys in (sc["keys1"], sc["keys2"]):
            pn, T = tv().normalize(keys)
            rpn, rT = ref_normalize(keys)
            assert same_bits(pn, rpn) and same_bits(T, rT)
            assert same_bits(tv().inv33(T), ref_inv33(T))
    rng = np.random.default_rng(1)
    for _ in range(200):
        S = rng.normal(0, 1, (3, 3)).astype(f32)
        assert same_bits(tv().inv33(S), ref_inv33(S))
    S = np.array([[1, 2, 3], [2, 4, 6], [0, 1, 5]], f32)             # det == 0 exactly: all zeros
    assert np.array_equal(tv().inv33(S), np.zeros((3, 3)))


def test_scores_and_masks_on_the_host_match_the_checker():
    n_nan = 0
    for i, sc in enumerate(scenes_for_the_checker()):
        N = len(sc["xy1"])
        a = tv().ransac_inputs(sc)
        sets = tv().random_sets(N, 24, i)
        sH, sF, H21, F21, mH, mF = tv().ransac_eval_host(*a, 1.0, sets)
        models = np.concatenate([H21, np.random.default_rng(i).normal(0, 1, (4, 3, 3)).astype(f32), np.zeros((1, 3, 3), f32)])
        for sigma in (1.0, 0.7):
            for model, M, ref in ((0, models, ref_check_h), (1, np.concatenate([F21, models[-5:]]), ref_check_f)):
                score, mask = tv().score_host(model, M, sc["xy1"], sc["xy2"], sigma)
                for k in range(len(M)):
                    rs, rm = ref(M[k], sc["xy1"], sc["xy2"], sigma)
                    assert same_bits(score[k], rs), (i, model, k, score[k], rs)
                    assert np.array_equal(mask[k], rm)
                    n_nan += bool(np.isnan(rs))
        # what ransac_eval_host reports for a hypothesis is the score of its own model
        assert same_bits(sH, tv().score_host(0, H21, sc["xy1"], sc["xy2"], 1.0)[0]) and same_bits(sF, tv().score_host(1, F21, sc["xy1"], sc["xy2"], 1.0)[0])
    assert n_nan > 0                                                     # the NaN scene and the zero model give NaN scores


def test_check_rt_on_the_host_matches_the_checker():
    seen = np.zeros(8, np.int64)
    for i, sc in enumerate(scenes_for_the_checker()):
        N = len(sc["xy1"])
        Rs, ts = tv().motion_hypotheses(sc, 8)
        rec = np.stack([tv().prepare_rt(sc["K"], Rs[q], ts[q]) for q in range(8)])
        for q in range(8):
            assert same_bits(rec[q], ref_prepare_rt(sc["K"], Rs[q], ts[q]))
        inl = np.random.default_rng(i).random(N) < 0.85
        for th2 in (4.0, 0.5):
            st, X, cp = tv().check_rt_host(rec, sc["K"], sc["xy1"], sc["xy2"], inl, th2)
            for q in range(8):
                rst, rX, rcp = ref_check_rt(rec[q], sc["K"], sc["xy1"], sc["xy2"], inl, th2)
                assert np.array_equal(st[q], rst), (i, q, np.nonzero(st[q] != rst)[0][:5])
                assert same_bits(X[q], rX) and same_bits(cp[q], rcp)
            seen += np.bincount(st.reshape(-1), minlength=8)
    assert (seen > 0).all(), seen


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the mirror against the literal sequence
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _acosf(x):
    libm = ctypes.CDLL("libm.so.6")
    libm.acosf.restype = ctypes.c_float; libm.acosf.argtypes = [ctypes.c_float]
    return f32(libm.acosf(float(x)))


def sequential_find(sc, sets, sigma, evaluate):
    """FindHomography / FindFundamental as the reference runs them: one iteration at a time, `if(currentScore>score)` from 0, vbMatchesInliers a copy"""
    a = tv().ransac_inputs(sc)
    N = len(sc["xy1"])
    out = {}
    for name, col in (("H", 0), ("F", 1)):
        score, best, M, inl = f32(0), -1, np.zeros((3, 3), f32), [False] * N
        for it in range(len(sets)):
            r = evaluate(a, sigma, sets[it:it + 1])
            cur, Mi, cur_inl = r[col][0], r[2 + col][0], r[4 + col][0]
            if cur > score:
                M = Mi.copy(); inl = list(cur_inl); score = cur; best = it
        out[name] = (score, best, M, np.array(inl))
    return out


def sequential_check_rt(sc, R, t, inliers, th2, evaluate):
    """CheckRT (:794-903) for one hypothesis around the per-match results"""
    rec = tv().prepare_rt(sc["K"], R, t)
    st, X, cp = (x[0] for x in evaluate(rec[None], sc["K"], sc["xy1"], sc["xy2"], inliers, th2))
    N1 = len(sc["keys1"])
    vbGood = [False] * N1; vP3D = np.zeros((N1, 3), f32); vCos = []; nGood = 0
    for i in range(len(st)):
        if not inliers[i]:
            continue
        if st[i] == 1:
            vbGood[sc["first"][i]] = False
            continue
        if st[i] < 6:
            continue
        vCos.append(cp[i]); vP3D[sc["first"][i]] = X[i]; nGood += 1
        if st[i] == 7:
            vbGood[sc["first"][i]] = True
    parallax = f32(0)
    if nGood > 0:
        vCos = np.sort(np.array(vCos, f32))
        parallax = f32(f64(_acosf(vCos[min(50, len(vCos) - 1)]) * f32(180)) / np.pi)
    return nGood, parallax, vP3D, np.array(vbGood)


def check_mirror(device, evaluate_ransac, evaluate_rt, cases=(("planar", 120, 31), ("general", 77, 32), ("general", 8, 33))):
    for kind, N, seed in cases:
        sc = tv().make_scene(kind, N, seed=seed, unmatched=N // 3, outliers=0.1)
        sets = tv().random_sets(N, 40, seed)
        m = tv().TwoViewInitializer(device, sc["K"], sc["keys1"], 1.0)
        got = m.find(sc["keys2"], sc["matches12"], sets)
        ref = sequential_find(sc, sets, 1.0, evaluate_ransac)
        for name in "HF":
            score, best, M, inl = ref[name]
            assert same_bits(got["S" + name], score) and got["best" + name] == best
            assert same_bits(got[name + "21"], M) and np.array_equal(got["inliers" + name], inl)
        assert same_bits(got["RH"], ref["H"][0] / (ref["H"][0] + ref["F"][0]))
        for n_hyp, inl in ((8, got["inliersH"]), (4, got["inliersF"]), (1, np.zeros(N, bool))):
            Rs, ts = tv().motion_hypotheses(sc, n_hyp)
            out = m.check_rt_batch(Rs, ts, inl, 4.0)
            for q in range(n_hyp):
                nGood, parallax, vP3D, vbGood = sequential_check_rt(sc, Rs[q], ts[q], inl, 4.0, evaluate_rt)
                assert out[q]["nGood"] == nGood and same_bits(out[q]["parallax"], parallax), (kind, q, out[q]["parallax"], parallax)
                assert same_bits(out[q]["vP3D"], vP3D) and np.array_equal(out[q]["vbGood"], vbGood)
        m.close()


def test_mirror_on_the_host_equals_the_literal_sequence():
    check_mirror(None, lambda a, sigma, sets: tv().ransac_eval_host(*a, sigma, sets), tv().check_rt_host)


def test_a_nan_or_zero_score_never_wins():
    sc = tv().make_scene("general", 30, seed=41)
    keys2 = sc["keys2"].copy(); keys2[sc["matches12"][sc["first"][0]]] = np.nan      # one match carries NaN: every score is NaN
    m = tv().TwoViewInitializer(None, sc["K"], sc["keys1"], 1.0)
    got = m.find(keys2, sc["matches12"], tv().random_sets(30, 10, 1))
    assert got["bestH"] == -1 and got["bestF"] == -1 and got["SH"] == 0 and got["SF"] == 0
    assert not got["inliersH"].any() and not got["inliersF"].any() and np.array_equal(got["H21"], np.zeros((3, 3))) and np.isnan(got["RH"])


def test_set_drawing_repeats_the_references_loop():
    rng = np.random.default_rng(7)
    for N in (8, 9, 200):
        raw = rng.integers(0, 2**31 - 1, 8 * 25, dtype=np.int64).astype(np.int32)
        got = tv().draw_sets(N, 25, raw)
        at = 0
        for it in range(25):
            avail = list(range(N))
            for j in range(8):
                randi = int((float(raw[at]) / (2147483647.0 + 1.0)) * len(avail)); at += 1
                assert got[it, j] == avail[randi]
                avail[randi] = avail[-1]; avail.pop()
        assert all(len(set(s)) == 8 for s in got.tolist())


def test_mirror_rejects_bad_arguments():
    from ccm_slam_amd._lib import CcmError
    sc = tv().make_scene("general", 20, seed=2)
    m = tv().TwoViewInitializer(None, sc["K"], sc["keys1"], 1.0)
    sets = tv().random_sets(20, 4, 0)
    bad = sets.copy(); bad[1, 3] = 20
    rep = sets.copy(); rep[2, 5] = rep[2, 0]
    few = sc["matches12"].copy(); few[sc["first"][:13]] = -1               # 7 matches left
    oob = sc["matches12"].copy(); oob[sc["first"][0]] = len(sc["keys2"])
    for keys2, m12, s in ((sc["keys2"], sc["matches12"], bad), (sc["keys2"], sc["matches12"], rep), (sc["keys2"], few, sets), (sc["keys2"], oob, sets)):
        with pytest.raises(CcmError):
            m.find(keys2, m12, s)
    with pytest.raises(CcmError):
        tv().draw_sets(7, 1, np.zeros(8, np.int32))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the branch
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 100, 300, 1000])
def test_planar_scene_takes_the_homography_and_the_general_scene_the_fundamental_matrix(N):
    for seed in (0, 1):
        r = {}
        for kind in ("planar", "general"):
            sc = tv().make_scene(kind, N, seed=seed)
            m = tv().TwoViewInitializer(None, sc["K"], sc["keys1"], 1.0)
            r[kind] = m.find(sc["keys2"], sc["matches12"], tv().random_sets(N, 200, seed))["RH"]
        print(f"N = {N} seed {seed}: RH planar {r['planar']:.3f}, general {r['general']:.3f}")
        assert r["planar"] > 0.40 and r["general"] < 0.40
