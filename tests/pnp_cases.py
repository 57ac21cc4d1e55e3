"""Shared by tests/test_pnp_cpu.py and tests/test_pnp_gpu.py: synthetic relocalisation candidates, a literal Python replay of cslam/src/PnPSolver.cpp (Python floats
in the reference's order of operations, numpy.float32 where the reference rounds to float, the legacy OpenCV calls restated as csrc/pnp_math.h states them) and a
literal sequential PnPsolver (SetRansacParameters, iterate, Refine) on a supplied array of raw rand() values."""
import math

import numpy as np

from ccm_slam_amd import pnp

RAND_MAX = 2147483647
DBL_EPSILON = 2.0 ** -52
DBL_MIN = 2.0 ** -1022
f32 = np.float32


# ---- IEEE helpers: Python raises where C returns inf / nan -------------------------------------------------------------------------------------
def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(x):
    if x != x or x < 0:
        return math.nan
    return math.sqrt(x)


# ---- the restated C-API calls --------------------------------------------------------------------------------------------------------------------
def cv_hypot(a, b):
    a = abs(a); b = abs(b)
    if a > b:
        b = _div(b, a)
        return a * _sqrt(1 + b * b)
    if b > 0:
        a = _div(a, b)
        return b * _sqrt(1 + a * a)
    return 0.0


def jacobi_svd(At, m, n, n1, want_vt=True):
    """JacobiSVDImpl_<double> on the n rows of At (m entries each, modified in place): returns (W, Vt)."""
    eps = DBL_EPSILON * 10
    W = []
    for i in range(n):
        sd = 0.0
        for k in range(m):
            sd += At[i][k] * At[i][k]
        W.append(sd)
    Vt = [[1.0 if i == k else 0.0 for k in range(n)] for i in range(n)] if want_vt else None
    for _ in range(max(m, 30)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                Ai, Aj = At[i], At[j]
                a, p, b = W[i], 0.0, W[j]
                for k in range(m):
                    p += Ai[k] * Aj[k]
                if abs(p) <= eps * _sqrt(a * b):
                    continue
                p *= 2
                beta = a - b
                gamma = cv_hypot(p, beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = _sqrt(_div(delta, gamma))
                    c = _div(p, gamma * s * 2)
                else:
                    c = _sqrt(_div(gamma + beta, gamma * 2))
                    s = _div(p, gamma * c * 2)
                a = b = 0.0
                for k in range(m):
                    t0 = c * Ai[k] + s * Aj[k]
                    t1 = -s * Ai[k] + c * Aj[k]
                    Ai[k] = t0; Aj[k] = t1
                    a += t0 * t0; b += t1 * t1
                W[i] = a; W[j] = b
                changed = True
                if Vt is not None:
                    Vi, Vj = Vt[i], Vt[j]
                    for k in range(n):
                        t0 = c * Vi[k] + s * Vj[k]
                        t1 = -s * Vi[k] + c * Vj[k]
                        Vi[k] = t0; Vj[k] = t1
        if not changed:
            break
    for i in range(n):
        sd = 0.0
        for k in range(m):
            sd += At[i][k] * At[i][k]
        W[i] = _sqrt(sd)
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            if Vt is not None:
                Vt[i], Vt[j] = Vt[j], Vt[i]
    rng = 0x12345678
    for i in range(n1):
        sd = W[i] if i < n else 0.0
        ii = 0
        while ii < 100 and sd <= DBL_MIN:
            val0 = 1.0 / m
            for k in range(m):
                rng = ((rng & 0xFFFFFFFF) * 4164903690 + (rng >> 32)) & 0xFFFFFFFFFFFFFFFF
                At[i][k] = val0 if (rng & 256) != 0 else -val0
            for _ in range(2):
                for j in range(i):
                    sd = 0.0
                    for k in range(m):
                        sd += At[i][k] * At[j][k]
                    asum = 0.0
                    for k in range(m):
                        t = At[i][k] - sd * At[j][k]
                        At[i][k] = t
                        asum += abs(t)
                    asum = _div(1, asum) if asum > eps * 100 else 0.0
                    for k in range(m):
                        At[i][k] *= asum
            sd = 0.0
            for k in range(m):
                sd += At[i][k] * At[i][k]
            sd = _sqrt(sd)
            ii += 1
        s = _div(1, sd) if sd > DBL_MIN else 0.0
        for k in range(m):
            At[i][k] *= s
    return W, Vt


def mul_transposed(A, rows, cols):
    D = [[0.0] * cols for _ in range(cols)]
    for i in range(cols):
        for j in range(i, cols):
            s = 0.0
            for k in range(rows):
                s += A[k][i] * A[k][j]
            D[i][j] = s
    for i in range(cols):
        for j in range(i + 1, cols):
            D[j][i] = D[i][j]
    return D


def svd_ut(A, n):
    """cvSVD(A, W, Ut, 0, MODIFY_A | U_T): (w, ut rows)"""
    At = [[A[k][i] for k in range(n)] for i in range(n)]
    W, _ = jacobi_svd(At, n, n, n, want_vt=False)
    return W, At


def invert3_svd(A):
    At = [[A[k][i] for k in range(3)] for i in range(3)]
    w, Vt = jacobi_svd(At, 3, 3, 3)
    X = [[0.0] * 3 for _ in range(3)]
    threshold = 0.0
    for i in range(3):
        threshold += w[i]
    threshold *= DBL_EPSILON * 2
    for i in range(3):
        wi = w[i]
        if abs(wi) <= threshold:
            continue
        wi = _div(1, wi)
        buf = [At[i][j] * wi for j in range(3)]
        for r in range(3):
            s = Vt[i][r]
            for j in range(3):
                X[r][j] = X[r][j] + s * buf[j]
    return X


def solve_svd(A, b, nc):
    At = [[A[k][i] for k in range(6)] for i in range(nc)]
    w, Vt = jacobi_svd(At, 6, nc, nc)
    x = [0.0] * nc
    threshold = 0.0
    for i in range(nc):
        threshold += w[i]
    threshold *= DBL_EPSILON * 2
    for i in range(nc):
        wi = w[i]
        if abs(wi) <= threshold:
            continue
        wi = _div(1, wi)
        s = 0.0
        for j in range(6):
            s += At[i][j] * b[j]
        s *= wi
        for j in range(nc):
            x[j] = x[j] + s * Vt[i][j]
    return x


# ---- PnPSolver.cpp, line by line -------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _dist2(p1, p2):
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2])


def qr_solve(A, b, X):
    """qr_solve (:851-941) on flat lists A (nr x nc), b, X; False at the singular exit (X untouched)."""
    nr, nc = 6, 4
    A1 = [0.0] * nr; A2 = [0.0] * nr
    kk = 0
    for k in range(nc):
        ik = kk
        eta = abs(A[ik])
        for i in range(k + 1, nr):
            elt = abs(A[ik])
            if eta < elt:
                eta = elt
            ik += nc
        if eta == 0:
            return False
        ik = kk; s = 0.0; inv_eta = 1.0 / eta
        for i in range(k, nr):
            A[ik] *= inv_eta
            s += A[ik] * A[ik]
            ik += nc
        sigma = _sqrt(s)
        if A[kk] < 0:
            sigma = -sigma
        A[kk] += sigma
        A1[k] = sigma * A[kk]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            ik = kk; s = 0.0
            for i in range(k, nr):
                s += A[ik] * A[ik + j - k]
                ik += nc
            tau = _div(s, A1[k])
            ik = kk
            for i in range(k, nr):
                A[ik + j - k] -= tau * A[ik]
                ik += nc
        kk += nc + 1
    jj = 0
    for j in range(nc):
        ij = jj; tau = 0.0
        for i in range(j, nr):
            tau += A[ij] * b[i]
            ij += nc
        tau = _div(tau, A1[j])
        ij = jj
        for i in range(j, nr):
            b[i] -= tau * A[ij]
            ij += nc
        jj += nc + 1
    X[nc - 1] = _div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        ij = i * nc + i + 1; s = 0.0
        for j in range(i + 1, nc):
            s += A[ij] * X[j]
            ij += 1
        X[i] = _div(b[i] - s, A2[i])
    return True


def compute_pose(pws, us, cam):
    """compute_pose (:468-516) on n correspondences: pws / us lists of n points (Python floats), cam = fu fv uc vc.  Returns (R 3x3, t, rep_errors[1..3], N)."""
    n = len(pws)
    fu, fv, uc, vc = (float(x) for x in cam)
    # choose_control_points
    cws = [[0.0] * 3 for _ in range(4)]
    for i in range(n):
        for j in range(3):
            cws[0][j] += pws[i][j]
    for j in range(3):
        cws[0][j] = cws[0][j] / n
    PW0 = [[pws[i][j] - cws[0][j] for j in range(3)] for i in range(n)]
    dc, uct = svd_ut(mul_transposed(PW0, n, 3), 3)
    for i in range(1, 4):
        k = _sqrt(dc[i - 1] / n)
        for j in range(3):
            cws[i][j] = cws[0][j] + k * uct[i - 1][j]
    # compute_barycentric_coordinates
    cc = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(1, 4):
            cc[i][j - 1] = cws[j][i] - cws[0][i]
    ci = invert3_svd(cc)
    alphas = []
    for i in range(n):
        pi = pws[i]
        a = [0.0] * 4
        for j in range(3):
            a[1 + j] = ci[j][0] * (pi[0] - cws[0][0]) + ci[j][1] * (pi[1] - cws[0][1]) + ci[j][2] * (pi[2] - cws[0][2])
        a[0] = 1.0 - a[1] - a[2] - a[3]
        alphas.append(a)
    # fill_M
    M = []
    for i in range(n):
        a = alphas[i]; u, v = us[i]
        M1 = [0.0] * 12; M2 = [0.0] * 12
        for k in range(4):
            M1[3 * k] = a[k] * fu; M1[3 * k + 1] = 0.0; M1[3 * k + 2] = a[k] * (uc - u)
            M2[3 * k] = 0.0; M2[3 * k + 1] = a[k] * fv; M2[3 * k + 2] = a[k] * (vc - v)
        M.append(M1); M.append(M2)
    _, ut = svd_ut(mul_transposed(M, 2 * n, 12), 12)
    # compute_L_6x10
    v = [ut[11], ut[10], ut[9], ut[8]]
    dv = [[None] * 6 for _ in range(4)]
    for i in range(4):
        a, b = 0, 1
        for j in range(6):
            dv[i][j] = [v[i][3 * a] - v[i][3 * b], v[i][3 * a + 1] - v[i][3 * b + 1], v[i][3 * a + 2] - v[i][3 * b + 2]]
            b += 1
            if b > 3:
                a += 1; b = a + 1
    L = []
    for i in range(6):
        L.append([_dot(dv[0][i], dv[0][i]), 2.0 * _dot(dv[0][i], dv[1][i]), _dot(dv[1][i], dv[1][i]), 2.0 * _dot(dv[0][i], dv[2][i]),
                  2.0 * _dot(dv[1][i], dv[2][i]), _dot(dv[2][i], dv[2][i]), 2.0 * _dot(dv[0][i], dv[3][i]), 2.0 * _dot(dv[1][i], dv[3][i]),
                  2.0 * _dot(dv[2][i], dv[3][i]), _dot(dv[3][i], dv[3][i])])
    rho = [_dist2(cws[0], cws[1]), _dist2(cws[0], cws[2]), _dist2(cws[0], cws[3]), _dist2(cws[1], cws[2]), _dist2(cws[1], cws[3]), _dist2(cws[2], cws[3])]

    def betas_1():
        b4 = solve_svd([[L[i][0], L[i][1], L[i][3], L[i][6]] for i in range(6)], rho, 4)
        if b4[0] < 0:
            b0 = _sqrt(-b4[0])
            return [b0, _div(-b4[1], b0), _div(-b4[2], b0), _div(-b4[3], b0)]
        b0 = _sqrt(b4[0])
        return [b0, _div(b4[1], b0), _div(b4[2], b0), _div(b4[3], b0)]

    def betas_2():
        b3 = solve_svd([[L[i][0], L[i][1], L[i][2]] for i in range(6)], rho, 3)
        if b3[0] < 0:
            be = [_sqrt(-b3[0]), _sqrt(-b3[2]) if b3[2] < 0 else 0.0]
        else:
            be = [_sqrt(b3[0]), _sqrt(b3[2]) if b3[2] > 0 else 0.0]
        if b3[1] < 0:
            be[0] = -be[0]
        return be + [0.0, 0.0]

    def betas_3():
        b5 = solve_svd([[L[i][0], L[i][1], L[i][2], L[i][3], L[i][4]] for i in range(6)], rho, 5)
        if b5[0] < 0:
            be = [_sqrt(-b5[0]), _sqrt(-b5[2]) if b5[2] < 0 else 0.0]
        else:
            be = [_sqrt(b5[0]), _sqrt(b5[2]) if b5[2] > 0 else 0.0]
        if b5[1] < 0:
            be[0] = -be[0]
        return be + [_div(b5[3], be[0]), 0.0]

    def gauss_newton(betas):
        x = [0.0] * 4
        for _ in range(5):
            A = [0.0] * 24; b = [0.0] * 6
            for i in range(6):
                r = L[i]
                A[4 * i] = 2 * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3]
                A[4 * i + 1] = r[1] * betas[0] + 2 * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3]
                A[4 * i + 2] = r[3] * betas[0] + r[4] * betas[1] + 2 * r[5] * betas[2] + r[8] * betas[3]
                A[4 * i + 3] = r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + 2 * r[9] * betas[3]
                b[i] = rho[i] - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] + r[2] * betas[1] * betas[1] + r[3] * betas[0] * betas[2] +
                                 r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] + r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] +
                                 r[8] * betas[2] * betas[3] + r[9] * betas[3] * betas[3])
            qr_solve(A, b, x)
            for i in range(4):
                betas[i] += x[i]

    def compute_R_and_t(betas):
        ccs = [[0.0] * 3 for _ in range(4)]
        for i in range(4):
            vv = ut[11 - i]
            for j in range(4):
                for k in range(3):
                    ccs[j][k] += betas[i] * vv[3 * j + k]
        pcs = []
        for i in range(n):
            a = alphas[i]
            pcs.append([a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j] for j in range(3)])
        if pcs[0][2] < 0.0:
            pcs = [[-p[0], -p[1], -p[2]] for p in pcs]
        # estimate_R_and_t
        pc0 = [0.0] * 3; pw0 = [0.0] * 3
        for i in range(n):
            for j in range(3):
                pc0[j] += pcs[i][j]
                pw0[j] += pws[i][j]
        for j in range(3):
            pc0[j] = pc0[j] / n
            pw0[j] = pw0[j] / n
        abt = [[0.0] * 3 for _ in range(3)]
        for i in range(n):
            pc, pw = pcs[i], pws[i]
            for j in range(3):
                abt[j][0] += (pc[j] - pc0[j]) * (pw[0] - pw0[0])
                abt[j][1] += (pc[j] - pc0[j]) * (pw[1] - pw0[1])
                abt[j][2] += (pc[j] - pc0[j]) * (pw[2] - pw0[2])
        At = [[abt[k][i] for k in range(3)] for i in range(3)]
        _, Vt = jacobi_svd(At, 3, 3, 3)
        U = [[At[k][i] for k in range(3)] for i in range(3)]
        V = [[Vt[k][i] for k in range(3)] for i in range(3)]
        R = [[_dot(U[i], V[j]) for j in range(3)] for i in range(3)]
        det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] - R[0][2] * R[1][1] * R[2][0] -
               R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
        if det < 0:
            R[2] = [-R[2][0], -R[2][1], -R[2][2]]
        t = [pc0[0] - _dot(R[0], pw0), pc0[1] - _dot(R[1], pw0), pc0[2] - _dot(R[2], pw0)]
        # reprojection_error
        sum2 = 0.0
        for i in range(n):
            pw = pws[i]
            Xc = _dot(R[0], pw) + t[0]
            Yc = _dot(R[1], pw) + t[1]
            inv_Zc = _div(1.0, _dot(R[2], pw) + t[2])
            ue = uc + fu * Xc * inv_Zc
            ve = vc + fv * Yc * inv_Zc
            u, v_ = us[i]
            sum2 += _sqrt((u - ue) * (u - ue) + (v_ - ve) * (v_ - ve))
        return R, t, sum2 / n

    sol = [None]
    for make in (betas_1, betas_2, betas_3):
        be = make()
        gauss_newton(be)
        sol.append(compute_R_and_t(be))
    N = 1
    if sol[2][2] < sol[1][2]:
        N = 2
    if sol[3][2] < sol[N][2]:
        N = 3
    return sol[N][0], sol[N][1], [sol[1][2], sol[2][2], sol[3][2]], N


def check_inliers(R, t, cam, P3Dw, P2D, max_err):
    """CheckInliers (:299-330) with the reference's mixed rounding: (mnInliersi, mask, error2 as float32)."""
    fu, fv, uc, vc = (float(x) for x in cam)
    mask, e2 = [], []
    with np.errstate(all="ignore"):
        for i in range(len(max_err)):
            x, y, z = (float(v) for v in P3Dw[i])
            Xc = f32(R[0][0] * x + R[0][1] * y + R[0][2] * z + t[0])
            Yc = f32(R[1][0] * x + R[1][1] * y + R[1][2] * z + t[1])
            invZc = f32(_div(1, R[2][0] * x + R[2][1] * y + R[2][2] * z + t[2]))
            ue = uc + fu * float(Xc) * float(invZc)
            ve = vc + fv * float(Yc) * float(invZc)
            distX = f32(float(P2D[i][0]) - ue)
            distY = f32(float(P2D[i][1]) - ve)
            error2 = f32(f32(distX * distX) + f32(distY * distY))
            e2.append(error2)
            mask.append(bool(error2 < f32(max_err[i])))
    return sum(mask), np.array(mask, bool), np.array(e2, np.float32)


def gather(cand, idx):
    """add_correspondence of the listed points: floats widened to doubles"""
    P3 = np.asarray(cand.P3Dw, np.float32).reshape(-1, 3); P2 = np.asarray(cand.P2D, np.float32).reshape(-1, 2)
    return [[float(v) for v in P3[i]] for i in idx], [[float(v) for v in P2[i]] for i in idx]


# ---- synthetic candidates ------------------------------------------------------------------------------------------------------------------------------
def rodrigues(a):
    a = np.asarray(a, np.float64); th = np.linalg.norm(a)
    if th == 0:
        return np.eye(3)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make_candidate(seed, n_true, n_out=0, cam=(500.0, 510.0, 320.0, 240.0), sigma2=1.0, shuffle=True, sparse=False):
    """n_true exact correspondences of a random pose (the projection rounded to f32) and n_out gross outliers displaced by 30 to 80 pixels.  meta holds the
    pose and which correspondences are true.  sparse: the correspondences sit at every other keypoint of a frame of 2 N + 3 keypoints."""
    rng = np.random.default_rng(seed)
    R = rodrigues(rng.uniform(-0.3, 0.3, 3)); t = rng.uniform(-0.3, 0.3, 3) + [0, 0, 0.5]
    N = n_true + n_out
    X = (rng.uniform(-1.5, 1.5, (N, 3)) + [0, 0, 5]).astype(np.float32)
    Xc = X.astype(np.float64) @ R.T + t
    uv = np.stack([cam[2] + cam[0] * Xc[:, 0] / Xc[:, 2], cam[3] + cam[1] * Xc[:, 1] / Xc[:, 2]], 1)
    true = np.zeros(N, bool); true[:n_true] = True
    ang = rng.uniform(0, 2 * np.pi, n_out); r = rng.uniform(30, 80, n_out)
    uv[n_true:] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1)
    if shuffle:
        p = rng.permutation(N)
        X, uv, true = X[p], uv[p], true[p]
    c = pnp.PnPCandidate(P3Dw=X, P2D=uv.astype(np.float32), sigma2=np.full(N, sigma2, np.float32), cam=cam)
    if sparse:
        c.n_matches = 2 * N + 3
        c.kp_idx = (2 * np.arange(N) + 1).astype(np.int32)
    c.meta = dict(R=R, t=t, true=true)
    return c


# ---- the sequential reference on supplied draws ------------------------------------------------------------------------------------------------------
class ArrayDraw:
    def __init__(self, raws):
        self.raws = [int(r) for r in raws]
        self.at = 0

    def __call__(self):
        v = self.raws[self.at]
        self.at += 1
        return v


def random_int(raw, d):
    return int((float(raw) / (float(RAND_MAX) + 1.0)) * d)


def to_tcw(Rt):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.asarray(Rt[:9], np.float64).reshape(3, 3).astype(np.float32)
    T[:3, 3] = np.asarray(Rt[9:], np.float64).astype(np.float32)
    return T


class RefSolver:
    """PnPsolver as the reference runs it, one hypothesis after the other: the constructor's SetRansacParameters (:111-147), iterate (:155-249), Refine (:251-296).
    compute_pose and CheckInliers of a hypothesis come from the host evaluator (one hypothesis per call), whose bits tests/test_pnp_cpu.py checks separately."""

    def __init__(self, cand, draw, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        self.c, self.draw, self.th2 = cand, draw, th2
        self.N = N = cand.N
        self.n_matches = cand.n_matches if cand.n_matches >= 0 else N
        self.kp = np.asarray(cand.kp_idx if cand.kp_idx is not None else np.arange(N))
        self.mRansacMinSet = minSet
        eps = f32(epsilon)
        nMin = int(f32(N) * eps)
        nMin = max(nMin, minInliers, minSet)
        self.mRansacMinInliers = nMin
        self.mRansacMaxIts = 1
        if N >= nMin:
            if eps < f32(nMin) / f32(N):
                eps = f32(nMin) / f32(N)
            nIt = 1 if nMin == N else int(math.ceil(math.log(1 - probability) / math.log(1 - float(eps) ** 3)))
            self.mRansacMaxIts = max(1, min(nIt, maxIterations))
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.mvbBestInliers = None
        self.mBestTcw = None
        self.n_refine_calls = 0
        self.refine_at_non_best = 0   # Refine() calls of hypotheses that reached the threshold without beating the best

    def Refine(self):
        self.n_refine_calls += 1
        n, inl, Rt = pnp.refine(self.c, self.mvbBestInliers, self.th2)
        self.mnRefinedInliers, self.mvbRefinedInliers = n, inl
        if n > self.mRansacMinInliers:
            self.mRefinedTcw = to_tcw(Rt)
            return True
        return False

    def _out(self, mask):
        vb = np.zeros(self.n_matches, bool)
        vb[self.kp[np.nonzero(mask)[0]]] = True
        return vb

    def iterate(self, nIterations):
        """(Tcw or None, bNoMore, vbInliers, nInliers)"""
        if self.N < self.mRansacMinInliers:
            return None, True, np.zeros(0, bool), 0
        nCurrentIterations = 0
        while self.mnIterations < self.mRansacMaxIts or nCurrentIterations < nIterations:
            nCurrentIterations += 1
            self.mnIterations += 1
            avail = list(range(self.N))
            idx = []
            for _ in range(self.mRansacMinSet):
                randi = random_int(self.draw(), len(avail))
                idx.append(avail[randi])
                avail[randi] = avail[-1]
                avail.pop()
            n_inl, Rt, masks = pnp.eval_hypotheses_host([self.c], [0], [idx], self.th2)
            if n_inl[0] >= self.mRansacMinInliers:
                if n_inl[0] > self.mnBestInliers:
                    self.mvbBestInliers = masks[0].copy()
                    self.mnBestInliers = int(n_inl[0])
                    self.mBestTcw = to_tcw(Rt[0])
                else:
                    self.refine_at_non_best += 1
                if self.Refine():
                    return self.mRefinedTcw.copy(), False, self._out(self.mvbRefinedInliers), self.mnRefinedInliers
        if self.mnIterations >= self.mRansacMaxIts:
            if self.mnBestInliers >= self.mRansacMinInliers:
                return self.mBestTcw.copy(), True, self._out(self.mvbBestInliers), self.mnBestInliers
            return None, True, np.zeros(0, bool), 0
        return None, False, np.zeros(0, bool), 0


def sequential_events(cands, raws, n_iterations=5, max_events=None, **params):
    """The round-robin `for each candidate not discarded: iterate(n)` until every candidate is discarded: the calls that returned a pose, as
    (cand, Tcw, vbInliers, nInliers, refined, bNoMore), the solvers, and the number of raw values consumed."""
    draw = ArrayDraw(raws)
    solvers = [RefSolver(c, draw, **params) for c in cands]
    discarded = [False] * len(cands)
    events = []
    while not all(discarded):
        for i, s in enumerate(solvers):
            if discarded[i]:
                continue
            Tcw, no_more, vb, n = s.iterate(n_iterations)
            if no_more:
                discarded[i] = True
            if Tcw is not None:
                events.append((i, Tcw, vb, n, not no_more, no_more))
                if max_events is not None and len(events) >= max_events:
                    return events, solvers, draw.at
    return events, solvers, draw.at
