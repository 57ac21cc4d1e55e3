"""Sim3 RANSAC on the device (ccm_sim3_ransac_eval, cslam::Sim3RansacBatch) against a literal restatement of cslam/src/Sim3Solver.cpp and of the
round-robin of LoopFinder::ComputeSim3 (LoopFinder.cpp:288-346).

The checker below restates every cv::Mat expression of Sim3Solver.cpp in float32 / float64 through numpy, with OpenCV 4.2 baseline-build
semantics (no HAVE_EIGEN, no FMA).  Where oracle/ref_shim/opencv2/mini_cv.h declares the semantics, the checker follows it:
  - `M = Pr2*Pr1.t()` (transposed operand): GEMMSingleMul<float, double>, double accumulator, rounded once    (mini_cv.h gemm_eval)
  - `mR12i*Pr2`, `Rcw*X + tcw`, `ms12i*mR12i*O2`: the small-matrix path, float accumulator, (float)(t*alpha + c*beta) in double  (gemm_eval)
  - `Pr1.dot(P3)`, `dist.dot(dist)`: double accumulation                                                       (Mat::dot)
  - `Mat * s`, `Mat / s`: x * (float)s in float                                                                 (operator*, operator/)
Restated here once, for OpenCV functions mini_cv.h does not carry:
  - cv::reduce(P, C, 1, REDUCE_SUM) on 3 columns: reduceC_<float, float, OpAdd<float>>, (s0 + s2) + s1 in float (reduce.cpp)
  - cv::pow(P3, 2): the product x*x in float (mathfuncs.cpp, ipower 2)
  - cv::eigen of the 4x4 float matrix: hal::Jacobi -> JacobiImpl_<float> with lapack.cpp's hypot, eps = FLT_EPSILON, at most 480 rotations,
    eigenvalues sorted descending (strict <) with the eigenvectors as rows (lapack.cpp)
  - cv::norm(vec) of a float row: normL2Sqr<float, double>, sqrt in double (stat.simd.hpp / norm.cpp)
  - `2*ang*vec/norm(vec)`: one MatOp_AddEx with alpha = (2*ang) * (1./norm), converted with (float)alpha (matop.cpp, cvt_32f)
  - cv::Rodrigues (cvRodrigues2, calibration.cpp): double, identity below DBL_EPSILON, R = (c*I + c1*r r^T) + s*[r]x, then float
  - `(1.0/ms12i)*mR12i.t()`: MatOp_T, transpose then convertTo with (float)(1.0/ms12i) unless that is 1 (matop.cpp)
  - `-sRinv*mt12i`: gemm with alpha = -1
The double-precision atan2 / sin / cos of the device library could differ from glibc's in the last bit; on every fixture here they do not,
so R, t and s are required to be identical (the tests print the largest difference).  The hypotheses of the per-hypothesis tests keep every
point's errors at least 1e-3 (relative) away from their thresholds (threshold_margin), so that such an ulp could not flip an inlier; the
schedule tests draw their samples from arrays and report that margin for an event whose mask differs.
"""
import ctypes
import functools
import itertools
import math
import threading

import numpy as np
import pytest

f32 = np.float32
RAND_MAX = 2147483647
FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)


# ---- the restated primitives ----------------------------------------------------------------------------------------------------------------------
def max_error_thresholds(sigma2):
    """mvnMaxError1/2.push_back(9.210*sigmaSquare): double product stored in a std::vector<size_t> (truncated)."""
    return np.array([int(9.210 * float(f32(s))) for s in np.atleast_1d(sigma2)], np.uint32)


def ransac_max_iterations(N, probability=0.99, min_inliers=6, max_iterations=300):
    """SetRansacParameters (Sim3Solver.cpp:94-118): mRansacMaxIts."""
    epsilon = f32(f32(min_inliers) / f32(N))
    if min_inliers == N:
        n_it = 1
    else:
        n_it = int(math.ceil(math.log(1 - probability) / math.log(1 - math.pow(float(epsilon), 3))))
    return max(1, min(n_it, max_iterations))


def random_int(raw, lo, hi):
    """DUtils::Random::RandomInt(min, max) = int(rand()/(RAND_MAX+1.0) * d) + min, d = max - min + 1."""
    d = hi - lo + 1
    return int((float(raw) / (float(RAND_MAX) + 1.0)) * d) + lo


def sample_indices(raws, N):
    """The three sample indices of one hypothesis: vAvailableIndices = mvAllIndices (identity), swap-with-back removal (:146-160)."""
    avail = list(range(N))
    out = []
    for r in raws:
        randi = random_int(r, 0, len(avail) - 1)
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


def cv_hypot(a, b):
    a, b = f32(abs(a)), f32(abs(b))
    if a > b:
        b = f32(b / a)
        return f32(a * f32(np.sqrt(f32(f32(1) + f32(b * b)))))
    if b > 0:
        a = f32(a / b)
        return f32(b * f32(np.sqrt(f32(f32(1) + f32(a * a)))))
    return f32(0)


def jacobi(A):
    """JacobiImpl_<float> of lapack.cpp on a symmetric n x n float matrix: (W descending, V rows = eigenvectors)."""
    n = A.shape[0]
    A = [f32(x) for x in np.asarray(A, np.float32).reshape(-1)]
    V = [f32(1) if i // n == i % n else f32(0) for i in range(n * n)]
    W = [f32(0)] * n
    indR, indC = [0] * n, [0] * n
    for k in range(n):
        W[k] = A[(n + 1) * k]
        if k < n - 1:
            m, mv = k + 1, abs(A[n * k + k + 1])
            for i in range(k + 2, n):
                if mv < abs(A[n * k + i]):
                    mv, m = abs(A[n * k + i]), i
            indR[k] = m
        if k > 0:
            m, mv = 0, abs(A[k])
            for i in range(1, k):
                if mv < abs(A[n * i + k]):
                    mv, m = abs(A[n * i + k]), i
            indC[k] = m
    for _ in range(n * n * 30):
        k, mv = 0, abs(A[indR[0]])
        for i in range(1, n - 1):
            if mv < abs(A[n * i + indR[i]]):
                mv, k = abs(A[n * i + indR[i]]), i
        l = indR[k]
        for i in range(1, n):
            if mv < abs(A[n * indC[i] + i]):
                mv, k, l = abs(A[n * indC[i] + i]), indC[i], i
        p = A[n * k + l]
        if abs(p) <= FLT_EPSILON:                              # NaN compares false: the rotations go on, as in C++
            break
        y = f32(float(f32(W[l] - W[k])) * 0.5)
        t = f32(abs(y) + cv_hypot(p, y))
        s = cv_hypot(p, t)
        c = f32(t / s)
        s = f32(p / s)
        t = f32(f32(p / t) * p)
        if y < 0:
            s, t = f32(-s), f32(-t)
        A[n * k + l] = f32(0)
        W[k] = f32(W[k] - t)
        W[l] = f32(W[l] + t)

        def rot(i0, i1, M):
            a0, b0 = M[i0], M[i1]
            M[i0] = f32(f32(a0 * c) - f32(b0 * s))
            M[i1] = f32(f32(a0 * s) + f32(b0 * c))
        for i in range(0, k):
            rot(n * i + k, n * i + l, A)
        for i in range(k + 1, l):
            rot(n * k + i, n * i + l, A)
        for i in range(l + 1, n):
            rot(n * k + i, n * l + i, A)
        for i in range(n):
            rot(n * k + i, n * l + i, V)
        for idx in (k, l):
            if idx < n - 1:
                m, mv = idx + 1, abs(A[n * idx + idx + 1])
                for i in range(idx + 2, n):
                    if mv < abs(A[n * idx + i]):
                        mv, m = abs(A[n * idx + i]), i
                indR[idx] = m
            if idx > 0:
                m, mv = 0, abs(A[idx])
                for i in range(1, idx):
                    if mv < abs(A[n * i + idx]):
                        mv, m = abs(A[n * i + idx]), i
                indC[idx] = m
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            for i in range(n):
                V[n * m + i], V[n * k + i] = V[n * k + i], V[n * m + i]
    return np.array(W, np.float32), np.array(V, np.float32).reshape(n, n)


def rodrigues(vec):
    """cv::Rodrigues of a float 3-vector into a float 3x3 (cvRodrigues2)."""
    rx, ry, rz = (float(v) for v in vec)
    theta = math.sqrt(rx * rx + ry * ry + rz * rz)
    if theta < DBL_EPSILON:
        return np.eye(3, dtype=np.float32)
    c, s = math.cos(theta), math.sin(theta)
    c1 = 1.0 - c
    itheta = 1.0 / theta if theta else 0.0
    rx, ry, rz = rx * itheta, ry * itheta, rz * itheta
    rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
    r_x = [0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0]
    return np.array([((1.0 if i % 4 == 0 else 0.0) * c + c1 * rrt[i]) + s * r_x[i] for i in range(9)], np.float64).astype(np.float32).reshape(3, 3)


def _small_gemm_row(a_row, b0, b1, b2, alpha=1.0, c=0.0):
    """small-matrix path, one output: float t = a0*b0 + a1*b1 + a2*b2, then (float)(t*alpha + c) in double."""
    t = f32(f32(f32(a_row[0] * b0) + f32(a_row[1] * b1)) + f32(a_row[2] * b2))
    return f32(float(t) * alpha + c)


def compute_sim3(x1, x2, fix_scale):
    """ComputeSim3(P1, P2) (Sim3Solver.cpp:213-321); x1, x2: (3 samples, 3) float32.  Returns R, t, s, sR, sRinv, tinv."""
    P1 = np.asarray(x1, np.float32).T       # columns = samples
    P2 = np.asarray(x2, np.float32).T
    third = f32(1.0 / 3)

    def centroid(P):
        C = np.array([f32(f32(f32(P[r, 0] + P[r, 2]) + P[r, 1]) * third) for r in range(3)], np.float32)   # reduce SUM, then C/P.cols
        return (P - C[:, None]).astype(np.float32), C
    Pr1, O1 = centroid(P1)
    Pr2, O2 = centroid(P2)
    M = np.zeros((3, 3), np.float32)
    for r in range(3):
        for c in range(3):
            acc = 0.0
            for k in range(3):
                acc += float(Pr2[r, k]) * float(Pr1[c, k])
            M[r, c] = f32(acc)
    m = lambda r, c: M[r, c]
    N11 = f32(f32(m(0, 0) + m(1, 1)) + m(2, 2)); N12 = f32(m(1, 2) - m(2, 1)); N13 = f32(m(2, 0) - m(0, 2)); N14 = f32(m(0, 1) - m(1, 0))
    N22 = f32(f32(m(0, 0) - m(1, 1)) - m(2, 2)); N23 = f32(m(0, 1) + m(1, 0)); N24 = f32(m(2, 0) + m(0, 2))
    N33 = f32(f32(-m(0, 0) + m(1, 1)) - m(2, 2)); N34 = f32(m(1, 2) + m(2, 1)); N44 = f32(f32(-m(0, 0) - m(1, 1)) + m(2, 2))
    Nm = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], np.float32)
    _, evec = jacobi(Nm)
    vec = evec[0, 1:4].copy()
    nrm = math.sqrt(sum(float(v) * float(v) for v in vec))
    ang = math.atan2(nrm, float(evec[0, 0]))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        alpha = f32(np.float64(2 * ang) * (np.float64(1.0) / np.float64(nrm)))
    vec = np.array([f32(f32(v * alpha) + f32(0)) for v in vec], np.float32)
    R = rodrigues(vec)
    P3 = np.array([[_small_gemm_row(R[r], Pr2[0, j], Pr2[1, j], Pr2[2, j]) for j in range(3)] for r in range(3)], np.float32)
    if not fix_scale:
        nom = 0.0
        for a, b in zip(Pr1.reshape(-1), P3.reshape(-1)):
            nom += float(a) * float(b)
        den = 0.0
        for a in P3.reshape(-1):
            den += float(f32(a * a))
        with np.errstate(divide="ignore", invalid="ignore"):
            s = f32(np.float64(nom) / np.float64(den))
    else:
        s = f32(1.0)
    t = np.array([_small_gemm_row(R[r], O2[0], O2[1], O2[2], -float(s), float(O1[r])) for r in range(3)], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        sR = (R * s + f32(0)).astype(np.float32)
        ainv = np.float64(1.0) / np.float64(s)
        sRi = R.T.copy() if ainv == 1.0 else (R.T * f32(ainv) + f32(0)).astype(np.float32)
    ti = np.array([_small_gemm_row(sRi[r], t[0], t[1], t[2], -1.0, 0.0) for r in range(3)], np.float32)
    return dict(R=R, t=t, s=s, sR=sR, sRi=sRi, ti=ti)


def _to_image(X, K):
    X = np.asarray(X, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        invz = (f32(1) / X[:, 2]).astype(np.float32)
    x, y = (X[:, 0] * invz).astype(np.float32), (X[:, 1] * invz).astype(np.float32)
    return (f32(K[0]) * x + f32(K[2])).astype(np.float32), (f32(K[1]) * y + f32(K[3])).astype(np.float32)


def _transform(Rm, tv, X):
    X = np.asarray(X, np.float32)
    out = []
    for r in range(3):
        acc = ((Rm[r, 0] * X[:, 0]).astype(np.float32) + (Rm[r, 1] * X[:, 1]).astype(np.float32)).astype(np.float32)
        acc = (acc + (Rm[r, 2] * X[:, 2]).astype(np.float32)).astype(np.float32)
        out.append((acc.astype(np.float64) + float(tv[r])).astype(np.float32))
    return np.stack(out, 1)


def check_inliers(hyp, X1, X2, K1, K2, thr1, thr2):
    """CheckInliers (Sim3Solver.cpp:324-348) with Project / FromCameraToImage: the inlier flags of every point."""
    with np.errstate(all="ignore"):
        p1u, p1v = _to_image(X1, K1)
        p2u, p2v = _to_image(X2, K2)
        u21, v21 = _to_image(_transform(hyp["sR"], hyp["t"], X2), K1)
        u12, v12 = _to_image(_transform(hyp["sRi"], hyp["ti"], X1), K2)
        d0, d1 = (p1u - u21).astype(np.float32), (p1v - v21).astype(np.float32)
        err1 = (d0.astype(np.float64) * d0 + d1.astype(np.float64) * d1).astype(np.float32)
        d0, d1 = (u12 - p2u).astype(np.float32), (v12 - p2v).astype(np.float32)
        err2 = (d0.astype(np.float64) * d0 + d1.astype(np.float64) * d1).astype(np.float32)
        return (err1 < np.asarray(thr1).astype(np.float32)) & (err2 < np.asarray(thr2).astype(np.float32)), err1, err2


def ref_hypothesis(cand, idx, fix_scale):
    X1, X2 = np.asarray(cand.X1, np.float32), np.asarray(cand.X2, np.float32)
    h = compute_sim3(X1[list(idx)], X2[list(idx)], fix_scale)
    inl, _, _ = check_inliers(h, X1, X2, cand.K1, cand.K2, cand.thr1, cand.thr2)
    return int(inl.sum()), h, inl


class RefSim3Solver:
    """Sim3Solver's RANSAC state and iterate() (Sim3Solver.cpp:94-191), drawing raw rand() values from `draw`."""

    def __init__(self, cand, fix_scale, probability=0.99, min_inliers=6, max_iterations=300, cache=None):
        self.c, self.fix = cand, fix_scale
        self.N = cand.N
        self.n1 = cand.n1 if cand.n1 >= 0 else cand.N
        self.idx1 = np.arange(cand.N) if cand.idx1 is None else np.asarray(cand.idx1)
        self.min_inl = min_inliers
        self.max_its = ransac_max_iterations(self.N, probability, min_inliers, max_iterations) if self.N >= min_inliers else 1
        self.its, self.best = 0, 0
        self.cache = {} if cache is None else cache

    def iterate(self, n, draw):
        if self.N < self.min_inl:
            return None, True
        cur = 0
        while self.its < self.max_its and cur < n:
            cur += 1
            self.its += 1
            idx = tuple(sample_indices([draw(), draw(), draw()], self.N))
            if idx not in self.cache:
                self.cache[idx] = ref_hypothesis(self.c, idx, self.fix)
            ni, h, inl = self.cache[idx]
            if ni >= self.best:
                self.best = ni
                if ni > self.min_inl:
                    vb = np.zeros(self.n1, bool)
                    vb[self.idx1[inl]] = True
                    return (h["R"], h["t"], h["s"], vb, ni, idx), False
        return None, self.its >= self.max_its


def ref_compute_sim3(cands, draw, fix_scale=False, accept=lambda k, ev: True, solver_iterations=5, **params):
    """The candidate loop of LoopFinder::ComputeSim3 (:288-346): events in order until `accept` takes one or every candidate is discarded."""
    solvers = [RefSim3Solver(c, fix_scale, **params) for c in cands]
    discarded = [False] * len(cands)
    n_cand = len(cands)
    events = []
    match = False
    while n_cand > 0 and not match:
        for i, S in enumerate(solvers):
            if discarded[i]:
                continue
            ev, no_more = S.iterate(solver_iterations, draw)
            if no_more:
                discarded[i] = True
                n_cand -= 1
            if ev is not None:
                events.append((i,) + ev)
                if accept(len(events) - 1, ev):
                    match = True
                    break
    return events


class ArrayDraw:
    def __init__(self, values):
        self.v, self.i = list(values), 0

    def __call__(self):
        x = self.v[self.i]
        self.i += 1
        return x


# ---- GPU tests ---------------------------------------------------------------------------------------------------------------------------------
def _cands(seed, n_true, n_false, n_points, outlier_frac=0.3, fix_scale=False):
    from ccm_slam_amd import sim3, synth
    return [sim3.Sim3Candidate(**d) for d in synth.make_sim3_candidates(seed, n_true, n_false, n_points, outlier_frac, fix_scale)]


def _ulp_diff(a, b):
    a = np.asarray(a, np.float32).reshape(-1); b = np.asarray(b, np.float32).reshape(-1)
    both_nan = np.isnan(a) & np.isnan(b)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia); ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    d = np.abs(ia - ib)
    d[both_nan] = 0
    d[(a == b)] = 0
    return d


_WORST = {"ulp": 0, "n_diff": 0}


def _compare_rts(rts, h):
    want = np.concatenate([h["R"].reshape(-1), h["t"], [h["s"]]]).astype(np.float32)
    d = _ulp_diff(rts, want)
    _WORST["ulp"] = max(_WORST["ulp"], int(d.max()))
    _WORST["n_diff"] += int((d > 0).sum())
    assert d.max() == 0, (rts, want, d)                       # measured: the device's atan2 / sin / cos agree with glibc's on every fixture


MARGIN = 1e-3


def threshold_margin(cand, idx, fix_scale):
    """the smallest |err - thr| / thr over the candidate's points and both errors of CheckInliers under the hypothesis (NaN errors compare false
    whatever the last bit, so they do not count)"""
    h = compute_sim3(np.asarray(cand.X1, np.float32)[list(idx)], np.asarray(cand.X2, np.float32)[list(idx)], fix_scale)
    _, e1, e2 = check_inliers(h, cand.X1, cand.X2, cand.K1, cand.K2, cand.thr1, cand.thr2)
    m = np.inf
    for e, t in ((e1, cand.thr1), (e2, cand.thr2)):
        t = np.asarray(t, np.float64)
        r = np.abs(e.astype(np.float64) - t) / t
        r = r[np.isfinite(r)]
        if r.size:
            m = min(m, float(r.min()))
    return m


def _random_hyps(rng, cands, H, fix_scale=False, pick=None):
    """H hypotheses whose every point keeps its errors at least MARGIN (relative) away from its thresholds, so that an ulp of the device's
    double atan2 / sin / cos could not flip an inlier.  pick(rng) -> (candidate, sample) proposes; proposals within the margin are dropped."""
    hc, hi = [], []
    while len(hc) < H:
        if pick is not None and len(hc) % 4 == 0:
            c, idx = pick(rng)
        else:
            c = int(rng.integers(0, len(cands)))
            idx = rng.choice(cands[c].N, 3, replace=False)
        if threshold_margin(cands[c], idx, fix_scale) < MARGIN:
            continue
        hc.append(c)
        hi.append(idx)
    return np.array(hc, np.int32), np.array(hi, np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("outlier_frac", [0.0, 0.3, 0.7])
def test_hypotheses_match_the_checker(ctx, fix_scale, outlier_frac):
    from ccm_slam_amd import sim3
    for seed, sizes in enumerate([[3, 6, 7, 20], [63, 64, 65], [200, 1000]]):
        cands = _cands(100 * seed + int(outlier_frac * 10) + 7 * fix_scale, 1, len(sizes) - 1, sizes, outlier_frac, fix_scale)
        rng = np.random.default_rng(seed)
        good = np.flatnonzero(~cands[0].meta["outlier"])
        # every fourth one a sample from the planted model of the true candidate, so that real inlier sets are exercised
        pick = (lambda r: (0, r.choice(good, 3, replace=False))) if good.size >= 3 else None
        hc, hi = _random_hyps(rng, cands, 40, fix_scale, pick)
        n, rts, masks = sim3.eval_hypotheses(ctx, cands, hc, hi, fix_scale)
        for h in range(len(hc)):
            ni, ref, inl = ref_hypothesis(cands[hc[h]], hi[h], fix_scale)
            assert n[h] == ni, (h, n[h], ni)
            assert np.array_equal(masks[h], inl)
            _compare_rts(rts[h], ref)
    print("largest R/t/s difference (f32 ulp):", _WORST)


@pytest.mark.gpu
def test_duplicated_points_give_nan_and_no_inliers(ctx):
    from ccm_slam_amd import sim3
    c = _cands(5, 1, 0, [30])[0]
    c.X1[3] = c.X1[2]; c.X1[4] = c.X1[2]; c.X2[3] = c.X2[2]; c.X2[4] = c.X2[2]
    n, rts, masks = sim3.eval_hypotheses(ctx, [c], [0, 0], [[2, 3, 4], [2, 3, 10]], False)
    ni, ref, inl = ref_hypothesis(c, [2, 3, 4], False)
    assert n[0] == 0 == ni and not masks[0].any()
    assert np.isnan(rts[0]).all() and np.isnan(ref["R"]).all()
    ni1, ref1, inl1 = ref_hypothesis(c, [2, 3, 10], False)
    assert n[1] == ni1 and np.array_equal(masks[1], inl1)
    _compare_rts(rts[1], ref1)


EDGE_N = (3, 4, 31, 32, 33, 63, 64, 65)
# checked on the CPU by test_edge_cases_have_samples_outside_the_margin.  N = 3 has a single triple: of the seeds 400 .. 419, its margin passes with all three
# points inliers at 403, 404, 410 .. 415 and 419, so 400 + N serves there too
EDGE_SEED = {N: 400 + N for N in EDGE_N}


@functools.lru_cache(maxsize=None)
def _edge_cases():
    """{N: (one true candidate of N correspondences, its samples that pass MARGIN)}: every triple proposed for N <= 4 (N = 3 has one), twelve drawn ones above"""
    out = {}
    for N in EDGE_N:
        c = _cands(EDGE_SEED[N], 1, 0, [N], 0.3)[0]
        rng = np.random.default_rng(N)
        proposals = list(itertools.combinations(range(N), 3)) if N <= 4 else [tuple(int(i) for i in rng.choice(N, 3, replace=False)) for _ in range(12)]
        out[N] = (c, [idx for idx in proposals if threshold_margin(c, idx, False) >= MARGIN])
    return out


def test_edge_cases_have_samples_outside_the_margin():
    assert all(len(ok) >= 1 for _, ok in _edge_cases().values()), {N: len(ok) for N, (_, ok) in _edge_cases().items()}


@pytest.mark.gpu
@pytest.mark.parametrize("N", EDGE_N)
def test_one_candidate_at_the_wave_block_and_mask_word_edges(ctx, N):
    """H = 1 (one wave), 4 (a whole workgroup) and 5 (one wave in a second workgroup); N around the 32-bit mask words and the 64-lane stride.  The mask buffer
    is filled with ones before the call: every word is written and no bit at or beyond N survives."""
    from ccm_slam_amd import sim3
    from ccm_slam_amd._lib import _p, check, lib
    assert all(len(ok) >= 1 for _, ok in _edge_cases().values())   # on the CPU, before any device call
    c, ok = _edge_cases()[N]
    pt_off, X1, X2, K1, K2, t1, t2, _, _ = sim3.pack([c])
    words = (N + 31) // 32
    for H in (1, 4, 5):
        hc = np.zeros(H, np.int32)
        hi = np.array([ok[h % len(ok)] for h in range(H)], np.int32)
        n_inl = np.zeros(H, np.int32); rts = np.zeros((H, 13), np.float32); mask_off = np.zeros(H + 1, np.int32)
        mask = np.full(H * words, 0xFFFFFFFF, np.uint32)
        check(lib().ccm_sim3_ransac_eval(ctx.handle, 1, _p(pt_off), _p(X1), _p(X2), _p(K1), _p(K2), _p(t1), _p(t2), H, _p(hc), _p(hi), 0, _p(n_inl), _p(rts),
                                         _p(mask_off), _p(mask)), ctx.handle)
        assert np.array_equal(mask_off, words * np.arange(H + 1))
        for h in range(H):
            bits = np.unpackbits(mask[words * h:words * (h + 1)].astype("<u4").view(np.uint8), bitorder="little")
            assert not bits[N:].any(), (N, H, h)
            ni, ref, inl = ref_hypothesis(c, hi[h], False)
            assert n_inl[h] == ni and np.array_equal(bits[:N].astype(bool), inl), (N, H, h, n_inl[h], ni)
            _compare_rts(rts[h], ref)


@pytest.mark.gpu
def test_drop_in_iterate_of_a_candidate_smaller_than_a_sample_fails_and_keeps_the_draws(ctx):
    """N = 2 with MinInliers = 2 reaches the evaluation, which has no row for such a candidate: the call fails (it always did: the entry point refuses N < 3) and
    the three values drawn for its one hypothesis are back in the thread's FIFO."""
    from ccm_slam_amd import sim3
    from ccm_slam_amd._lib import CcmError
    sim3.clear_draws()
    s = sim3.Sim3Solver(_cands(54, 1, 0, [2])[0], min_inliers=2)
    with pytest.raises(CcmError):
        s.iterate(5)
    assert sim3.draws_pending().size == 3
    sim3.clear_draws()


def _run_batch(cands, draws, fix_scale=False, reject=0, **kw):
    from ccm_slam_amd import sim3
    b = sim3.Sim3Ransac(cands, fix_scale=fix_scale, draws=draws, **kw)
    evs = []
    while True:
        e = b.next()
        if e is None:
            break
        evs.append(e)
        if len(evs) > reject:
            break
    st = b.stats()
    b.close()
    return evs, st


def _check_schedule(cands, draws, fix_scale=False, reject=0, **kw):
    from ccm_slam_amd import sim3
    sim3.clear_draws()
    got, st = _run_batch(cands, draws, fix_scale, reject, **kw)
    ad = ArrayDraw(draws)
    want = ref_compute_sim3(cands, ad, fix_scale, accept=lambda k, ev: k >= reject,
                            **{k: v for k, v in kw.items() if k in ("min_inliers", "max_iterations", "probability", "solver_iterations")})
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert g[0] == w[0] and g[5] == w[5], ("inlier count", g[5], w[5], "threshold margin", threshold_margin(cands[w[0]], w[6], fix_scale))
        assert np.array_equal(g[4], w[4]), ("mask", "threshold margin", threshold_margin(cands[w[0]], w[6], fix_scale))
        _compare_rts(np.concatenate([g[1].reshape(-1), g[2], [g[3]]]), dict(R=w[1], t=w[2], s=w[3]))
    pending = sim3.draws_pending()
    assert st[0] - len(pending) == ad.i                        # the values the sequential reference consumed
    assert np.array_equal(pending, np.asarray(draws[ad.i:ad.i + len(pending)], np.int32))   # and the FIFO holds the next ones
    sim3.clear_draws()
    return got, want, st


def _draws(seed, n=40000):
    return np.random.default_rng(seed).integers(0, RAND_MAX + 1, n, dtype=np.int64).astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("reject", [0, 1, 3])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_schedule_matches_the_literal_round_robin(ctx, seed, reject):
    rng = np.random.default_rng(seed)
    K = int(rng.integers(1, 11))
    sizes = [int(x) for x in rng.integers(7, 60, K)]
    sizes[-1] = 4                                              # N < MinInliers: discarded with no draw
    if K > 2:
        sizes[1] = 6                                           # N == MinInliers: one iteration, never a success
    n_true = max(1, K // 3)
    cands = _cands(seed + 50, n_true, K - n_true, sizes, outlier_frac=0.5)
    got, want, st = _check_schedule(cands, _draws(seed), reject=reject, max_iterations=60)
    assert st[2] >= 1


@pytest.mark.gpu
def test_schedule_all_candidates_fail(ctx):
    cands = _cands(11, 0, 4, [30, 12, 25, 9], outlier_frac=1.0)
    got, want, st = _check_schedule(cands, _draws(11))
    assert got == [] and st[2] == 1                           # no success: one pass evaluates the whole schedule
    assert st[1] == sum(ransac_max_iterations(c.N) for c in cands if c.N >= 6)


@pytest.mark.gpu
def test_success_on_the_last_allowed_iteration(ctx):
    """A candidate whose call returns a Sim3 on its last allowed iteration is discarded at its next call, with no draw (bNoMore)."""
    from ccm_slam_amd import sim3
    cands = _cands(21, 1, 1, [12, 15], outlier_frac=0.0)
    # max_iterations = 1: the true candidate's first hypothesis is its last allowed one; the verifier rejects it and the loop goes on
    got, want, st = _check_schedule(cands, _draws(21, 4000), reject=3, max_iterations=1)
    assert len(got) == 1 and got[0][0] == 0
    assert st[0] == 6                                         # one hypothesis per candidate, and none for the discarded winner


@pytest.mark.gpu
def test_glibc_stream(ctx):
    """srand(seed), then the batch with its default source (the C library's rand()), against the checker drawing libc.rand after the same srand."""
    from ccm_slam_amd import sim3
    libc = ctypes.CDLL(None)
    cands = _cands(31, 1, 3, [40, 25, 30, 22], outlier_frac=0.4)
    sim3.clear_draws()
    libc.srand(1234)
    got, st = _run_batch(cands, None, reject=1, max_iterations=80)
    pending = sim3.draws_pending()
    libc.srand(1234)
    n_used = [0]

    def draw():
        n_used[0] += 1
        return libc.rand()
    want = ref_compute_sim3(cands, draw, False, accept=lambda k, ev: k >= 1, max_iterations=80)
    assert len(got) == len(want) and all(g[0] == w[0] and g[5] == w[5] and np.array_equal(g[4], w[4]) for g, w in zip(got, want))
    assert st[0] - len(pending) == n_used[0]
    assert np.array_equal(pending, np.array([libc.rand() for _ in range(len(pending))], np.int32))
    sim3.clear_draws()


@pytest.mark.gpu
def test_two_threads_with_their_own_fifo(ctx):
    from ccm_slam_amd import sim3
    cands_a = _cands(41, 1, 2, [30, 20, 25], outlier_frac=0.5)
    cands_b = _cands(42, 1, 3, [22, 35, 18, 40], outlier_frac=0.5)
    da, db = _draws(41), _draws(42)

    def run(cands, d):
        sim3.clear_draws()
        out = []
        for _ in range(2):                                     # two batches: the second starts with the FIFO the first left
            evs, st = _run_batch(cands, d, reject=1)
            out.append(([(e[0], e[5], e[1].tobytes(), e[4].tobytes()) for e in evs], st))
        out.append(sim3.draws_pending().tolist())
        sim3.clear_draws()
        return out
    solo = [run(cands_a, da), run(cands_b, db)]
    res = [None, None]

    def worker(k, cands, d):
        res[k] = run(cands, d)
    th = [threading.Thread(target=worker, args=(0, cands_a, da)), threading.Thread(target=worker, args=(1, cands_b, db))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert res[0] == solo[0] and res[1] == solo[1]


@pytest.mark.gpu
def test_error_paths(ctx):
    from ccm_slam_amd import sim3
    from ccm_slam_amd._lib import CcmError
    cands = _cands(51, 1, 0, [10])
    with pytest.raises(CcmError):
        sim3.eval_hypotheses(ctx, cands, [0], [[0, 1, 10]])        # index >= N
    with pytest.raises(CcmError):
        sim3.eval_hypotheses(ctx, cands, [0], [[0, 1, 1]])         # repeated index
    with pytest.raises(CcmError):
        sim3.eval_hypotheses(ctx, cands, [1], [[0, 1, 2]])         # candidate out of range
    small = _cands(52, 1, 0, [2])
    with pytest.raises(CcmError):
        sim3.eval_hypotheses(ctx, small, [0], [[0, 1, 0]])         # N < 3
    n, rts, masks = sim3.eval_hypotheses(ctx, cands, np.zeros(0, np.int32), np.zeros((0, 3), np.int32))
    assert n.size == 0
    from ccm_slam_amd._lib import lib
    assert lib().ccm_sim3_ransac_eval(ctx.handle, 1, None, None, None, None, None, None, None, 0, None, None, 0, None, None, None, None) == -1
    # the batch: the supplied draws run out before the reference would stop
    b = sim3.Sim3Ransac(_cands(53, 0, 2, [20, 20], outlier_frac=1.0), draws=_draws(53, 10))
    with pytest.raises(CcmError):
        while b.next() is not None:
            pass
    b.close()
    sim3.clear_draws()
    with pytest.raises(CcmError):
        sim3.Sim3Ransac(cands, solver_iterations=0)


@pytest.mark.gpu
def test_chain_with_optimize_sim3(ctx):
    """A true synthetic loop: the RANSAC estimate, fed to ccm_sim3_optimize, reaches the planted Sim3 (tolerances of tests/test_sim3_gpu.py)."""
    from ccm_slam_amd import optimizer, sim3, synth
    p = synth.make_sim3_problem(150, 0)
    _, _, s2, _ = synth.scale_tables()
    rng = np.random.default_rng(0)
    oc1, oc2 = rng.integers(0, 3, 150), rng.integers(0, 3, 150)
    c = sim3.Sim3Candidate(X1=p["P1c"].astype(np.float32), X2=p["P2c"].astype(np.float32), thr1=sim3.max_error_thresholds(s2[oc1]),
                           thr2=sim3.max_error_thresholds(s2[oc2]), K1=p["K1"], K2=p["K2"])
    sim3.clear_draws()
    b = sim3.Sim3Ransac([c], draws=_draws(7))
    ev = b.next()
    b.close()
    sim3.clear_draws()
    assert ev is not None and ev[0] == 0 and ev[5] > 6          # the first hypothesis with more than MinInliers inliers is returned
    R, t, s = ev[1].astype(np.float64), ev[2].astype(np.float64), ev[3]
    q = synth.quat_from_R(R[None])[0]
    s0 = np.concatenate([q, t, [s]])
    out, inl, nin = optimizer.sim3_optimization(ctx, s0, p["P1c"], p["P2c"], p["obs1"], p["obs2"], p["info1"], p["info2"], p["K1"], p["K2"], p["th2"], False)
    gt = p["gt_sim3"]
    assert nin > 100
    assert np.abs(out[4:7] - gt[4:7]).max() < min(0.05, np.abs(t - gt[4:7]).max()) and abs(out[7] - gt[7]) < 0.02
    assert min(np.abs(out[:4] - gt[:4]).max(), np.abs(out[:4] + gt[:4]).max()) < 0.01
    assert (inl[p["is_outlier"]] == 0).mean() > 0.9


@pytest.mark.gpu
def test_drop_in_solver_iterate_matches_the_reference(ctx):
    """Sim3Solver::iterate(5) as shim/Sim3Solver_hip.cpp runs it (ccmh_sim3_solver_iterate: one launch per call, rand() through the thread's
    FIFO), round-robin over candidates as LoopFinder::ComputeSim3 calls it, against the checker's Sim3Solver on the same glibc stream."""
    from ccm_slam_amd import sim3
    libc = ctypes.CDLL(None)
    for seed, sizes, frac in ((61, [40, 25, 6, 4, 30], 0.4), (62, [18, 22], 0.0)):
        cands = _cands(seed, 1, len(sizes) - 1, sizes, outlier_frac=frac)
        sim3.clear_draws()
        libc.srand(seed)
        dev = [sim3.Sim3Solver(c, max_iterations=60) for c in cands]
        got = []
        live = list(range(len(cands)))
        while live and len([g for g in got if g[1]]) < 2:
            for i in list(live):
                ok, no_more, best, n = dev[i].iterate(5)
                got.append((i, ok, no_more, tuple(dev[i].state), best if ok else None, n if ok else 0))
                if no_more:
                    live.remove(i)
        pending = sim3.draws_pending()
        libc.srand(seed)
        used = [0]

        def draw():
            used[0] += 1
            return libc.rand()
        ref = [RefSim3Solver(c, False, max_iterations=60) for c in cands]
        for i, ok, no_more, state, best, n in got:
            ev, rno_more = ref[i].iterate(5, draw)
            assert (ev is not None) == ok and rno_more == no_more and state == (ref[i].its, ref[i].best), (i, ok, no_more, state, ref[i].its, ref[i].best)
            if ok:
                R, t, s, inl = best
                assert n == ev[4]
                _compare_rts(np.concatenate([R.reshape(-1), t, [s]]), dict(R=ev[0], t=ev[1], s=ev[2]))
                vb = np.zeros(ref[i].n1, bool)
                vb[ref[i].idx1[inl]] = True
                assert np.array_equal(vb, ev[3])
        assert any(g[1] for g in got)
        assert np.array_equal(pending, np.array([libc.rand() for _ in range(len(pending))], np.int32))
        sim3.clear_draws()
