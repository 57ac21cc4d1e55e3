"""Extended-precision reference of one Levenberg-Marquardt trial of the bundle adjustment, written from the formulas
(g2o's EdgeSE3ProjectXYZ, RobustKernelHuber, BlockSolver's Schur complement, SE3Quat::exp), not from ba.hip or
oracle/ba_ref.cpp.  numpy.longdouble throughout (64-bit mantissa on x86: `HAVE_EXTENDED`); plain array code, clarity
over speed.  No GPU, no oracle.

The reference knows nothing about the device's layout: cameras are named by their index in the problem, landmarks
likewise, off-diagonal blocks by the pair (camera i < camera j).  Tests map it into whatever order the device uses.

    lin = linearize(prob, cam_qt, pt_xyz)            per-observation residuals, Jacobians, Huber weights
    sys = reduced_system(prob, lam, ...)             Hpp, Hll, b, W, D^-1, S (no lambda on its diagonal), b_schur,
                                                     |S|_acc, |b|_acc, term counts, cond(D), max diagonal
    stp = lm_step(prob, sys, lam)                    dx_c, dx_l, new state, new chi2, per-edge chi2, depth sign
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble
HAVE_EXTENDED = np.finfo(LD).nmant >= 63
U53 = 2.0 ** -53
COND_KNEE = 1e8          # landmarks whose cond(D) exceeds this enter the bounds multiplied by cond(D) / COND_KNEE


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def huber_dsqr(delta: float) -> float:
    """The g2o fork keeps delta^2 in a float member: threshold and outlier constant are (double)(float)(delta * delta)."""
    return float(np.float32(np.float64(delta) * np.float64(delta)))


def huber(e2, delta: float):
    """(rho0, rho1) of RobustKernelHuber::robustify for an array of squared errors; delta <= 0: no kernel."""
    e2 = np.asarray(e2, dtype=LD)
    if not delta > 0:
        return e2.copy(), np.ones_like(e2)
    dsqr = LD(huber_dsqr(delta))
    d = LD(np.float64(delta))
    inl = e2 <= dsqr
    s = np.sqrt(np.where(inl, LD(1), e2))
    return np.where(inl, e2, 2 * s * d - dsqr), np.where(inl, LD(1), d / s)


def rot_from_quat(q):
    """Rotation matrices (n, 3, 3) of quaternions (n, 4) = (x, y, z, w), normalised first (SE3Quat's constructor)."""
    q = np.asarray(q, dtype=LD)
    q = q / np.sqrt((q * q).sum(1))[:, None]
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3), LD)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - w * z); R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y); R[:, 2, 1] = 2 * (y * z + w * x); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def quat_from_rot(R):
    """Unit quaternion (x, y, z, w), w >= 0, of ONE 3x3 matrix by the trace method (what Eigen's Quaterniond(R) computes; the
    matrix of SE3Quat::exp's small-angle branch is not exactly orthogonal and goes through the same formulas)."""
    R = np.asarray(R, dtype=LD)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4, LD)
    if t > 0:
        s = np.sqrt(t + 1)
        q[3] = s / 2
        s = LD(0.5) / s
        q[0] = (R[2, 1] - R[1, 2]) * s; q[1] = (R[0, 2] - R[2, 0]) * s; q[2] = (R[1, 0] - R[0, 1]) * s
    else:
        i = int(np.argmax([R[0, 0], R[1, 1], R[2, 2]]))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1)
        q[i] = s / 2
        s = LD(0.5) / s
        q[3] = (R[k, j] - R[j, k]) * s; q[j] = (R[j, i] + R[i, j]) * s; q[k] = (R[k, i] + R[i, k]) * s
    q = q / np.sqrt((q * q).sum())
    return -q if q[3] < 0 else q


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=LD)


def se3_exp(u):
    """SE3Quat::exp of u = (omega, upsilon): (quaternion xyzw, translation).  Below theta = 1e-5 g2o takes R = I + Om + Om^2 and V = R."""
    u = np.asarray(u, dtype=LD)
    om, up = u[:3], u[3:]
    th = np.sqrt((om * om).sum())
    Om = skew(om)
    Om2 = Om @ Om
    I = np.eye(3, dtype=LD)
    if th < LD(0.00001):
        R = I + Om + Om2
        V = R
    else:
        s, c = np.sin(th), np.cos(th)
        R = I + s / th * Om + (1 - c) / (th * th) * Om2
        V = I + (1 - c) / (th * th) * Om + (th - s) / (th * th * th) * Om2
    return quat_from_rot(R), V @ up


def se3_log(q, t):
    """Inverse of se3_exp for a rotation well away from pi: u = (omega, upsilon) with exp(u) = (q, t)."""
    q = np.asarray(q, dtype=LD); t = np.asarray(t, dtype=LD)
    q = q / np.sqrt((q * q).sum())
    if q[3] < 0:
        q = -q
    n = np.sqrt((q[:3] * q[:3]).sum())
    th = 2 * np.arctan2(n, q[3])
    om = q[:3] * (th / n) if n > 0 else np.zeros(3, LD)
    Om = skew(om)
    I = np.eye(3, dtype=LD)
    if th < LD(1e-6):
        V = I + Om / 2 + (Om @ Om) / 6
    else:
        V = I + (1 - np.cos(th)) / (th * th) * Om + (th - np.sin(th)) / (th * th * th) * (Om @ Om)
    return np.concatenate([om, _solve3(V, t)])


def _solve3(A, b):
    """3x3 solve by cofactors in long double"""
    A = np.asarray(A, dtype=LD)
    c = np.empty((3, 3), LD)
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]; s = [k for k in range(3) if k != j]
            c[i, j] = (-1) ** (i + j) * (A[r[0], s[0]] * A[r[1], s[1]] - A[r[0], s[1]] * A[r[1], s[0]])
    det = (A[0] * c[0]).sum()
    return (c.T @ np.asarray(b, dtype=LD)) / det


def quat_mul(a, b):
    ax, ay, az, aw = a; bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], dtype=LD)


def oplus(u, cam):
    """VertexSE3Expmap::oplusImpl: exp(u) * T for one pose (7,) = (qx, qy, qz, qw, tx, ty, tz)."""
    cam = np.asarray(cam, dtype=LD)
    qe, te = se3_exp(u)
    Re = rot_from_quat(qe[None])[0]
    q = quat_mul(qe, cam[:4] / np.sqrt((cam[:4] * cam[:4]).sum()))
    q = q / np.sqrt((q * q).sum())
    if q[3] < 0:
        q = -q
    return np.concatenate([q, te + Re @ cam[4:]])


def residuals(cam_qt, cam_K, pt_xyz, e_cam, e_pt, e_obs):
    """Xc = R X + t, e = obs - K proj(Xc) of the given observations: (Xc (m, 3), e (m, 2), R (m, 3, 3))."""
    R = rot_from_quat(_ld(cam_qt)[:, :4])[e_cam]
    t = _ld(cam_qt)[e_cam, 4:]
    X = _ld(pt_xyz)[e_pt]
    K = _ld(cam_K)[e_cam]
    Xc = np.einsum("nij,nj->ni", R, X) + t
    proj = np.stack([Xc[:, 0] / Xc[:, 2] * K[:, 0] + K[:, 2], Xc[:, 1] / Xc[:, 2] * K[:, 1] + K[:, 3]], 1)
    return Xc, _ld(e_obs) - proj, R


def jacobians(Xc, R, K):
    """EdgeSE3ProjectXYZ::linearizeOplus: Ji = d e / d point (m, 2, 3), Jj = d e / d pose (m, 2, 6), pose = (rotation, translation)."""
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    fx, fy = K[:, 0], K[:, 1]
    m = Xc.shape[0]
    tmp = np.zeros((m, 2, 3), LD)
    tmp[:, 0, 0] = fx; tmp[:, 0, 2] = -x / z * fx
    tmp[:, 1, 1] = fy; tmp[:, 1, 2] = -y / z * fy
    Ji = -(1 / z)[:, None, None] * np.einsum("nij,njk->nik", tmp, R)
    Jj = np.zeros((m, 2, 6), LD)
    z2 = z * z
    Jj[:, 0, 0] = x * y / z2 * fx; Jj[:, 0, 1] = -(1 + x * x / z2) * fx; Jj[:, 0, 2] = y / z * fx
    Jj[:, 0, 3] = -1 / z * fx; Jj[:, 0, 5] = x / z2 * fx
    Jj[:, 1, 0] = (1 + y * y / z2) * fy; Jj[:, 1, 1] = -x * y / z2 * fy; Jj[:, 1, 2] = -x / z * fy
    Jj[:, 1, 4] = -1 / z * fy; Jj[:, 1, 5] = y / z2 * fy
    return Ji, Jj


def active_edges(prob, e_level=None, pt_lo=None, pt_hi=None):
    lvl = prob.get("e_level") if e_level is None else e_level
    act = np.ones(int(prob["n_edge"]), bool) if lvl is None else np.asarray(lvl) == 0
    if pt_lo is not None:
        p = np.asarray(prob["e_pt"])
        act &= (p >= pt_lo) & (p < pt_hi)
    return np.flatnonzero(act)


def linearize(prob, cam_qt=None, pt_xyz=None, e_level=None, huber_delta=None, edges=None):
    """Residual, Jacobians and robust weight of every active (level 0) observation at the given state.  Keys: edges (indices into
    the problem's arrays), Xc, e, Ji, Jj, e2 = info |e|^2, rho0, rho1, w = rho1 info, chi2 = sum rho0."""
    cam_qt = prob["cam_qt"] if cam_qt is None else cam_qt
    pt_xyz = prob["pt_xyz"] if pt_xyz is None else pt_xyz
    delta = float(prob["huber_delta"]) if huber_delta is None else float(huber_delta)
    idx = active_edges(prob, e_level) if edges is None else np.asarray(edges)
    ec, ep = np.asarray(prob["e_cam"])[idx], np.asarray(prob["e_pt"])[idx]
    Xc, e, R = residuals(cam_qt, prob["cam_K"], pt_xyz, ec, ep, np.asarray(prob["e_obs"])[idx])
    Ji, Jj = jacobians(Xc, R, _ld(prob["cam_K"])[ec])
    info = _ld(prob["e_info"])[idx]
    e2 = info * (e * e).sum(1)
    rho0, rho1 = huber(e2, delta)
    return dict(edges=idx, e_cam=ec, e_pt=ep, Xc=Xc, e=e, Ji=Ji, Jj=Jj, info=info, e2=e2, rho0=rho0, rho1=rho1, w=rho1 * info,
                chi2=rho0.sum())


def _sym3_inv(D):
    """Inverse of symmetric 3x3 matrices (n, 3, 3) by cofactors"""
    a, b, c = D[:, 0, 0], D[:, 0, 1], D[:, 0, 2]
    d, e, f = D[:, 1, 1], D[:, 1, 2], D[:, 2, 2]
    c00, c01, c02 = d * f - e * e, e * c - b * f, b * e - d * c
    det = c00 * a + c01 * b + c02 * c
    out = np.empty_like(D)
    out[:, 0, 0] = c00; out[:, 0, 1] = out[:, 1, 0] = c01; out[:, 0, 2] = out[:, 2, 0] = c02
    out[:, 1, 1] = a * f - c * c; out[:, 1, 2] = out[:, 2, 1] = c * b - a * e; out[:, 2, 2] = a * d - b * b
    return out / det[:, None, None]


def _add_at(n, idx, vals):
    out = np.zeros((n,) + vals.shape[1:], LD)
    np.add.at(out, idx, vals)
    return out


def reduced_system(prob, lam, cam_qt=None, pt_xyz=None, e_level=None, huber_delta=None, pt_lo=None, pt_hi=None):
    """The normal equations of the active observations and their Schur complement onto the free cameras, at damping `lam`.

    With pt_lo / pt_hi only the observations of landmarks pt_lo <= p < pt_hi contribute (one rank's part of a sharded build);
    the set of free cameras is that of the whole problem either way.

    cams        free cameras that have an active observation, ascending problem index (n_c)
    pts         landmarks with a contributing observation, ascending (n_l)
    Hpp, b_p    (n_c, 6, 6), (n_c, 6);   Hll, b_l: (n_l, 3, 3), (n_l, 3)
    W           (m, 6, 3) Hpl block of every contributing observation of a free camera: w_cam, w_pt index cams / pts, w_edge the problem
    Dinv, condD (n_l, 3, 3), (n_l,)      D = Hll + lam I
    blk_ij      (n_b, 2) block pattern of S: the n_c diagonal blocks first, then every pair i < j (indices into cams) that shares a landmark
    S, S_abs    (n_b, 6, 6) blocks of Hpp - sum W D^-1 W^T WITHOUT lam on the diagonal; the same sums over the absolute values of
                every elementary product, the terms of landmarks with cond(D) > COND_KNEE scaled by cond(D) / COND_KNEE
    S_n         (n_b,) terms per entry (observations of the camera + pair instances of the block);  S_wide (n_b,) a widened term entered
    b, b_abs    (n_c, 6) b_p - sum W D^-1 b_l, ditto;  b_n, b_wide (n_c,)
    max_diag    largest diagonal entry of Hpp and Hll (computeLambdaInit runs over every vertex)
    """
    cam_fixed = np.asarray(prob["cam_fixed"]).astype(bool)
    lin = linearize(prob, cam_qt, pt_xyz, e_level, huber_delta)
    free_has = np.zeros(int(prob["n_cam"]), bool)
    free_has[lin["e_cam"]] = True
    cams = np.flatnonzero(free_has & ~cam_fixed)
    if pt_lo is not None:
        keep = (lin["e_pt"] >= pt_lo) & (lin["e_pt"] < pt_hi)
        lin = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == keep.shape else v) for k, v in lin.items()}
        lin["chi2"] = lin["rho0"].sum()
    cam_idx = -np.ones(int(prob["n_cam"]), np.int64); cam_idx[cams] = np.arange(cams.size)
    pts = np.unique(lin["e_pt"])
    pt_idx = -np.ones(int(prob["n_pt"]), np.int64); pt_idx[pts] = np.arange(pts.size)
    Ji, Jj, w, e = lin["Ji"], lin["Jj"], lin["w"], lin["e"]
    aJi, aJj, ae = np.abs(Ji), np.abs(Jj), np.abs(e)
    lp = pt_idx[lin["e_pt"]]
    n_l, n_c = pts.size, cams.size
    # landmark side: every active observation, fixed cameras included
    Hll = _add_at(n_l, lp, w[:, None, None] * np.einsum("nki,nkj->nij", Ji, Ji))
    b_l = _add_at(n_l, lp, -w[:, None] * np.einsum("nki,nk->ni", Ji, e))
    b_l_abs = _add_at(n_l, lp, w[:, None] * np.einsum("nki,nk->ni", aJi, ae))
    k_l = np.bincount(lp, minlength=n_l)
    D = Hll + LD(lam) * np.eye(3, dtype=LD)
    Dinv = _sym3_inv(D)
    ev = np.linalg.eigvalsh(D.astype(np.float64)) if n_l else np.zeros((0, 3))
    condD = np.abs(ev).max(1) / np.abs(ev).min(1) if n_l else np.zeros(0)
    wide = np.maximum(condD / COND_KNEE, 1.0).astype(LD)
    # camera side: observations of free cameras only
    fr = np.flatnonzero(cam_idx[lin["e_cam"]] >= 0)
    cf, lf = cam_idx[lin["e_cam"][fr]], lp[fr]
    Hpp_e = w[fr, None, None] * np.einsum("nki,nkj->nij", Jj[fr], Jj[fr])
    Hpp = _add_at(n_c, cf, Hpp_e)
    Hpp_abs = _add_at(n_c, cf, w[fr, None, None] * np.einsum("nki,nkj->nij", aJj[fr], aJj[fr]))
    b_p = _add_at(n_c, cf, -w[fr, None] * np.einsum("nki,nk->ni", Jj[fr], e[fr]))
    b_p_abs = _add_at(n_c, cf, w[fr, None] * np.einsum("nki,nk->ni", aJj[fr], ae[fr]))
    W = w[fr, None, None] * np.einsum("nki,nkj->nij", Jj[fr], Ji[fr])
    aW = w[fr, None, None] * np.einsum("nki,nkj->nij", aJj[fr], aJi[fr])
    n_cam_edges = np.bincount(cf, minlength=n_c)
    # b_schur
    Y = np.einsum("nij,njk->nik", W, Dinv[lf])                     # W D^-1
    aY = np.einsum("nij,njk->nik", aW, np.abs(Dinv[lf]))
    b = b_p - _add_at(n_c, cf, np.einsum("nij,nj->ni", Y, b_l[lf]))
    b_abs = b_p_abs + _add_at(n_c, cf, wide[lf, None] * np.einsum("nij,nj->ni", aY, b_l_abs[lf]))
    # terms of one entry of b: one per observation in b_p, one per observation in the Schur sum, and b_l inside such a term is itself a
    # sum over the landmark's observations (the longest one counts)
    k_max = np.zeros(n_c, np.int64)
    np.maximum.at(k_max, cf, k_l[lf])
    b_n = 2 * n_cam_edges + k_max
    b_wide = np.zeros(n_c, bool); b_wide[cf[wide[lf] > 1]] = True
    # pair instances: per landmark every (a, c) of its free-camera observations with camera(a) <= camera(c)
    order = np.lexsort((cf, lf))
    lf_s, cf_s = lf[order], cf[order]
    starts = np.flatnonzero(np.r_[True, lf_s[1:] != lf_s[:-1]]) if fr.size else np.zeros(0, np.int64)
    lens = np.diff(np.r_[starts, lf_s.size])
    pa, pc = [], []
    for ln in np.unique(lens):
        st = starts[lens == ln]
        ia, ic = np.triu_indices(int(ln))
        pa.append((st[:, None] + ia[None]).ravel()); pc.append((st[:, None] + ic[None]).ravel())
    pa = order[np.concatenate(pa)] if pa else np.zeros(0, np.int64)
    pc = order[np.concatenate(pc)] if pc else np.zeros(0, np.int64)
    key = cf[pa] * max(n_c, 1) + cf[pc]
    off_keys = np.unique(key[cf[pa] != cf[pc]])
    blk_ij = np.concatenate([np.stack([np.arange(n_c), np.arange(n_c)], 1), np.stack([off_keys // max(n_c, 1), off_keys % max(n_c, 1)], 1)]).astype(np.int64)
    all_keys = blk_ij[:, 0] * max(n_c, 1) + blk_ij[:, 1]
    srt = np.argsort(all_keys)
    blk_of = srt[np.searchsorted(all_keys[srt], key)]
    n_b = blk_ij.shape[0]
    S = np.zeros((n_b, 6, 6), LD); S_abs = np.zeros((n_b, 6, 6), LD)
    S[:n_c] = Hpp; S_abs[:n_c] = Hpp_abs
    CH = 200000
    for s0 in range(0, pa.size, CH):
        a, c, bk = pa[s0:s0 + CH], pc[s0:s0 + CH], blk_of[s0:s0 + CH]
        np.subtract.at(S, bk, np.einsum("nik,njk->nij", Y[a], W[c]))
        np.add.at(S_abs, bk, wide[lf[a], None, None] * np.einsum("nik,njk->nij", aY[a], aW[c]))
    S_n = np.bincount(blk_of, minlength=n_b).astype(np.int64)
    S_n[:n_c] += n_cam_edges
    S_wide = np.zeros(n_b, bool); S_wide[blk_of[wide[lf[pa]] > 1]] = True
    inst_n = np.bincount(blk_of, minlength=n_b).astype(np.int64)
    md = LD(0)
    if n_c:
        md = max(md, np.abs(np.einsum("nii->ni", Hpp)).max())
    if n_l:
        md = max(md, np.abs(np.einsum("nii->ni", Hll)).max())
    return dict(lin=lin, cams=cams, pts=pts, cam_idx=cam_idx, pt_idx=pt_idx, Hpp=Hpp, b_p=b_p, Hll=Hll, b_l=b_l, b_l_abs=b_l_abs, k_l=k_l,
                W=W, W_abs=aW, w_cam=cf, w_pt=lf, w_edge=lin["edges"][fr], Dinv=Dinv, condD=condD, wide=wide, blk_ij=blk_ij, S=S, S_abs=S_abs, S_n=S_n,
                S_wide=S_wide, inst_n=inst_n, pair_a=pa, pair_c=pc, pair_blk=blk_of, b=b, b_abs=b_abs, b_n=np.asarray(b_n, np.int64) + np.zeros(n_c, np.int64),
                b_wide=b_wide, max_diag=md, lam=lam)


def dense(sys, lam=0.0, what="S"):
    """The reduced matrix as one symmetric array (6 n_c, 6 n_c), lam added to the diagonal."""
    n_c = sys["cams"].size
    A = np.zeros((6 * n_c, 6 * n_c), LD)
    for (i, j), B in zip(sys["blk_ij"], sys[what]):
        A[6 * i:6 * i + 6, 6 * j:6 * j + 6] = B
        if i != j:
            A[6 * j:6 * j + 6, 6 * i:6 * i + 6] = B.T
    return A + LD(lam) * np.eye(6 * n_c, dtype=LD)


def solve_refined(A, b, rounds=3):
    """f64 solve + iterative refinement with the residual in long double"""
    A64 = A.astype(np.float64)
    x = np.linalg.solve(A64, b.astype(np.float64)).astype(LD)
    for _ in range(rounds):
        r = b - A @ x
        x = x + np.linalg.solve(A64, r.astype(np.float64)).astype(LD)
    return x


def landmark_step(sys, dx_c):
    """dx_l = D^-1 (b_l - W^T dx_c) for a given camera step (n_c, 6); also the same sum over absolute values and its term count."""
    n_l = sys["pts"].size
    dx_c = np.asarray(dx_c, dtype=LD).reshape(-1, 6)
    t = np.einsum("nij,ni->nj", sys["W"], dx_c[sys["w_cam"]])
    rhs = sys["b_l"] - _add_at(n_l, sys["w_pt"], t)
    rhs_abs = sys["b_l_abs"] + _add_at(n_l, sys["w_pt"], np.einsum("nij,ni->nj", sys["W_abs"], np.abs(dx_c[sys["w_cam"]])))
    dx_l = np.einsum("nij,nj->ni", sys["Dinv"], rhs)
    dx_l_abs = sys["wide"][:, None] * np.einsum("nij,nj->ni", np.abs(sys["Dinv"]), rhs_abs)
    return dx_l, dx_l_abs, 2 * sys["k_l"]


def apply_step(prob, sys, dx_c, dx_l, cam_qt=None, pt_xyz=None):
    cam = _ld(prob["cam_qt"] if cam_qt is None else cam_qt).copy()
    cam[:, :4] /= np.sqrt((cam[:, :4] ** 2).sum(1))[:, None]
    pts = _ld(prob["pt_xyz"] if pt_xyz is None else pt_xyz).copy()
    dx_c = np.asarray(dx_c, dtype=LD).reshape(-1, 6)
    for k, c in enumerate(sys["cams"]):
        cam[c] = oplus(dx_c[k], cam[c])
    pts[sys["pts"]] += dx_l
    return cam, pts


def lm_step(prob, sys, lam, cam_qt=None, pt_xyz=None, e_level=None, huber_delta=None, dx_c=None):
    """One LM trial on `sys` (built at the same state and lam): the exact step unless dx_c is given; new state; robust chi2, per-edge
    chi2 = info |e|^2 and depth sign of every active observation at the new state; computeScale's denominator (without the 1e-3)."""
    n_c = sys["cams"].size
    if dx_c is None:
        dx_c = solve_refined(dense(sys, lam), sys["b"].ravel()).reshape(n_c, 6) if n_c else np.zeros((0, 6), LD)
    dx_c = np.asarray(dx_c, dtype=LD).reshape(n_c, 6)
    dx_l, dx_l_abs, dx_l_n = landmark_step(sys, dx_c)
    cam, pts = apply_step(prob, sys, dx_c, dx_l, cam_qt, pt_xyz)
    lin = linearize(prob, cam, pts, e_level, huber_delta)
    scale = (dx_c * (LD(lam) * dx_c + sys["b_p"])).sum() + (dx_l * (LD(lam) * dx_l + sys["b_l"])).sum()
    return dict(dx_c=dx_c, dx_l=dx_l, dx_l_abs=dx_l_abs, dx_l_n=dx_l_n, cam=cam, pts=pts, chi2=lin["chi2"], edge_chi2=lin["e2"], edges=lin["edges"],
                depth_pos=lin["Xc"][:, 2] > 0, scale=scale, lin=lin)


def next_lambda(lam, chi_before, chi_after, scale):
    """Levenberg update of an accepted trial (optimization_algorithm_levenberg.cpp): lambda *= max(1/3, min(2/3, 1 - (2 rho - 1)^3))"""
    rho = (LD(chi_before) - LD(chi_after)) / (LD(scale) + LD(1e-3))
    alpha = min(1 - (2 * rho - 1) ** 3, LD(2) / 3)
    return LD(lam) * max(LD(1) / 3, alpha), rho


def camera_centres_and_rotations(cam):
    R = rot_from_quat(np.asarray(cam, dtype=LD)[:, :4])
    return -np.einsum("nji,nj->ni", R, np.asarray(cam, dtype=LD)[:, 4:]), R


def pose_distance(cam_a, cam_b):
    """per pose: distance of the camera centres (m) and rotation angle between them (rad), long double"""
    ca, Ra = camera_centres_and_rotations(cam_a)
    cb, Rb = camera_centres_and_rotations(cam_b)
    dR = np.einsum("nij,nkj->nik", Ra, Rb)
    # angle from the antisymmetric part (accurate for small angles, unlike acos of the trace)
    v = np.stack([dR[:, 2, 1] - dR[:, 1, 2], dR[:, 0, 2] - dR[:, 2, 0], dR[:, 1, 0] - dR[:, 0, 1]], 1) / 2
    return np.sqrt(((ca - cb) ** 2).sum(1)), np.arcsin(np.minimum(np.sqrt((v * v).sum(1)), LD(1)))


# ---- the accumulation bound -----------------------------------------------------------------------------------------------------
# An entry that is a sum of n terms, accumulated in f64 in ANY order, errs by at most about n 2^-53 sum|term|; c more units cover the
# rounding inside one term (residual, projection, Jacobians, Huber weight, 3x3 inverse, two small products).  S_abs / b_abs are the same
# sums as S / b with the absolute value of every factor of every term (|Jj|, |Ji|, |e|, |W|, |D^-1|, |b_l|_acc).
#
# C_ORACLE is MEASURED: the largest |S_oracle - S_ref| / (2^-53 |S|_acc) - n (and the same for b) of oracle.ba_partial_system (f64, g2o's
# operation order, not the code under test) over the problems and dampings of tests/test_ba_reference_cpu.py:
#     python -m tests.test_ba_reference_cpu        ->  largest c over S: 455.6, over b: 274.4     (x86-64, 80-bit long double)
# rounded up to 500.  It is dominated by the residual, a difference of about one pixel between pixel coordinates of several hundred: its
# relative error of a few hundred 2^-53 goes into b directly and into S through the weight delta / sqrt(e2) of Huber's outlier branch.
# The device gets 4 x that: it uses one reciprocal where g2o divides twelve times, fused multiply-adds, and another summation tree.
C_ORACLE = 500
C_DEVICE = 4 * C_ORACLE
WIDE_SHARE_CAP = 0.02     # at most this share of the entries of a case may have a bound widened by cond(D) > COND_KNEE


def bound_S(sys, c, lam_on_diag=0.0):
    """per block (n_b, 6, 6): (n + c) 2^-53 |S|_acc; with lam_on_diag the diagonal carries lam as one more term"""
    acc = sys["S_abs"].copy()
    n = sys["S_n"].astype(LD)[:, None, None] + np.zeros((1, 6, 6), LD)
    if lam_on_diag:
        n_c = sys["cams"].size
        acc[:n_c] += LD(lam_on_diag) * np.eye(6, dtype=LD)
        n[:n_c] += np.eye(6, dtype=LD)
    return (n + c) * LD(U53) * acc


def bound_b(sys, c):
    return (sys["b_n"].astype(LD)[:, None] + c) * LD(U53) * sys["b_abs"]


def wide_share(sys):
    """share of the entries of [S | b] whose bound was widened by an ill-conditioned landmark"""
    n = 36 * sys["S_wide"].size + 6 * sys["b_wide"].size
    return (36 * sys["S_wide"].sum() + 6 * sys["b_wide"].sum()) / max(n, 1)


def planted_huber_problem(rel, delta=None):
    """Three cameras with identity rotation and power-of-two intrinsics in front of 14 landmarks; camera 1's observation of landmark 0 has the
    residual (1, 0) EXACTLY (the projection is exact in f64) and the information dsqr (1 + rel), so e2 = dsqr (1 + rel) with
    dsqr = (double)(float)(delta^2): rel = 0 sits on the threshold, +-2^-30 on either side.  Returns (problem, index of that observation)."""
    delta = float(np.float32(np.sqrt(np.float32(5.991)))) if delta is None else delta
    rng = np.random.default_rng(7)
    n_cam, n_pt = 3, 14
    cam = np.zeros((n_cam, 7)); cam[:, 3] = 1.0
    cam[:, 4:7] = [[0.25, 0, 0], [0, 0, 0], [-0.25, 0.125, 0]]
    K = np.tile([512.0, 512.0, 256.0, 256.0], (n_cam, 1))
    pts = np.column_stack([rng.uniform(-1, 1, n_pt), rng.uniform(-0.7, 0.7, n_pt), rng.uniform(2, 4, n_pt)])
    pts[0] = [0.5, 0.25, 2.0]
    e_cam = np.repeat(np.arange(n_cam, dtype=np.int32), n_pt)
    e_pt = np.tile(np.arange(n_pt, dtype=np.int32), n_cam)
    Xc = pts[e_pt] + cam[e_cam, 4:7]
    obs = np.column_stack([512 * Xc[:, 0] / Xc[:, 2] + 256, 512 * Xc[:, 1] / Xc[:, 2] + 256]) + rng.normal(0, 1.5, (e_cam.size, 2))
    info = np.ones(e_cam.size)
    k = int(np.flatnonzero((e_cam == 1) & (e_pt == 0))[0])
    obs[k] = [512 * 0.25 + 256 + 1.0, 512 * 0.125 + 256]
    info[k] = huber_dsqr(delta) * (1.0 + rel)
    fixed = np.zeros(n_cam, np.uint8); fixed[0] = 1
    return {"n_cam": n_cam, "n_pt": n_pt, "n_edge": int(e_cam.size), "cam_qt": cam, "cam_fixed": fixed, "cam_K": K, "pt_xyz": pts,
            "e_cam": e_cam, "e_pt": e_pt, "e_obs": obs, "e_info": info, "e_level": np.zeros(e_cam.size, np.uint8), "huber_delta": delta}, k
