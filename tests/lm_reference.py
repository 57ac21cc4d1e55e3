"""Extended-precision reference of ONE linearisation of the motion-only pose optimisation (poseopt.hip): per-edge residual and Huber terms, the normal
equations H (upper triangle, 21 entries) and b (6) in the order the kernel keeps them (acc[0..20]: rows of the upper triangle; acc[21..26]), the robust
chi2, and the absolute-value accumulations the error bounds are stated in.  Written from the formulas (g2o's EdgeSE3ProjectXYZOnlyPose, RobustKernelHuber),
not from the kernel.  Plain numpy; the SAME code runs in numpy.longdouble (the truth) and in numpy.float64 (the yardstick for what f64 arithmetic costs:
C_F64 below).  The second half does the same for OptimizeSim3 (sim3opt.hip) with the reference's numeric Jacobians.  No GPU, no library call.

tests/ba_reference.py holds the same formulas fixed to long double; it supplies `_ld`, `U53`, `HAVE_EXTENDED` and `huber_dsqr` here, and
tests/test_lm_reference_cpu.py checks that rot / huber / jacobian below reproduce its rot_from_quat / huber / jacobians exactly in long double.
"""
from __future__ import annotations

import numpy as np

from tests.ba_reference import HAVE_EXTENDED, LD, U53, _ld, huber_dsqr   # noqa: F401  (re-exported for the tests)

HUBER_DELTA = float(np.float32(np.sqrt(np.float64(5.991))))   # Optimizer.cpp:236: const float deltaMono = sqrt(5.991)
H_SLOTS = [(r, c) for r in range(6) for c in range(r, 6)]     # acc[k] = H[r, c]


def rot(q, dt):
    """rotation matrix of ONE quaternion (x, y, z, w), normalised first"""
    q = np.asarray(q, dtype=dt)
    x, y, z, w = q / np.sqrt((q * q).sum())
    one, two = dt(1), dt(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=dt)


def huber(e2, robust, dt, delta=HUBER_DELTA):
    """(rho0, rho1) of RobustKernelHuber::robustify per edge; edges with robust == 0 have no kernel.  The g2o fork keeps delta^2 in a float member."""
    dsqr, d = dt(huber_dsqr(delta)), dt(delta)
    out = (np.asarray(robust) != 0) & (e2 > dsqr)
    s = np.sqrt(np.where(out, e2, dt(1)))
    return np.where(out, dt(2) * s * d - dsqr, e2), np.where(out, d / s, dt(1))


def jacobian(Xc, K, dt):
    """EdgeSE3ProjectXYZOnlyPose::linearizeOplus: d e / d (omega, upsilon) of the left-multiplied increment, [n, 2, 6]"""
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    fx, fy = dt(K[0]), dt(K[1])
    z2 = z * z
    J = np.zeros((Xc.shape[0], 2, 6), dt)
    J[:, 0, 0] = x * y / z2 * fx; J[:, 0, 1] = -(dt(1) + x * x / z2) * fx; J[:, 0, 2] = y / z * fx
    J[:, 0, 3] = -dt(1) / z * fx; J[:, 0, 5] = x / z2 * fx
    J[:, 1, 0] = (dt(1) + y * y / z2) * fy; J[:, 1, 1] = -x * y / z2 * fy; J[:, 1, 2] = -x / z * fy
    J[:, 1, 4] = -dt(1) / z * fy; J[:, 1, 5] = y / z2 * fy
    return J


def pose_linearise(cam_qt, Xw, obs, info, K, level=None, robust=None, dtype=LD):
    """One linearisation at cam_qt (qx qy qz qw tx ty tz) of the edges with level == 0, Huber on the edges with robust != 0.

    active   indices of the active edges;  n_act
    e        [n_act, 2] obs - K proj(R X + t);  e2 = info |e|^2;  rho, w (Huber rho0, rho1)
    J        [n_act, 2, 6]
    H        [21] sum w info J_r J_c over both rows, slots H_SLOTS;  b [6] = -sum w info J_r e
    H_abs    [21] sum |J_r| w info |J_c|;  b_abs [6] sum |J_r| |w info e|     (every elementary product, absolute)
    chi2     sum rho
    """
    dt = dtype
    n = np.asarray(Xw).shape[0]
    level = np.zeros(n, np.uint8) if level is None else np.asarray(level)
    robust = np.ones(n, np.uint8) if robust is None else np.asarray(robust)
    act = np.flatnonzero(level == 0)
    cam = np.asarray(cam_qt, np.float64).astype(dt)
    Kd = np.asarray(K, np.float64).astype(dt)
    X = np.asarray(Xw, np.float64).astype(dt)[act]
    o = np.asarray(obs, np.float64).astype(dt)[act]
    om = np.asarray(info, np.float64).astype(dt)[act]
    Xc = X @ rot(cam[:4], dt).T + cam[4:]
    proj = np.stack([Xc[:, 0] / Xc[:, 2] * Kd[0] + Kd[2], Xc[:, 1] / Xc[:, 2] * Kd[1] + Kd[3]], 1)
    e = o - proj
    e2 = om * (e * e).sum(1)
    rho, w = huber(e2, robust[act], dt)
    J = jacobian(Xc, Kd, dt)
    wom = w * om
    aJ, ae = np.abs(J), np.abs(e)
    H = np.array([(wom[:, None] * J[:, :, r] * J[:, :, c]).sum() for r, c in H_SLOTS], dtype=dt)
    H_abs = np.array([(wom[:, None] * aJ[:, :, r] * aJ[:, :, c]).sum() for r, c in H_SLOTS], dtype=dt)
    b = np.array([-(wom[:, None] * J[:, :, r] * e).sum() for r in range(6)], dtype=dt)
    b_abs = np.array([(wom[:, None] * aJ[:, :, r] * ae).sum() for r in range(6)], dtype=dt)
    return dict(active=act, n_act=int(act.size), Xc=Xc, e=e, e2=e2, rho=rho, w=w, info=om, J=J, H=H, b=b, H_abs=H_abs, b_abs=b_abs, chi2=rho.sum(),
                obs=o, K=Kd)


def full_H(H21):
    H = np.zeros((6, 6), np.asarray(H21).dtype)
    for k, (r, c) in enumerate(H_SLOTS):
        H[r, c] = H[c, r] = H21[k]
    return H


# ---- the accumulation bound ----------------------------------------------------------------------------------------------------------------------------------
# A sum of n terms accumulated in f64 in ANY order errs by at most about n 2^-53 sum|term|; c more units cover the roundings inside one term (rotation,
# projection, residual — a difference of about a pixel between pixel coordinates of several hundred —, Jacobian, Huber weight, the products).
#
# C_F64 is MEASURED on the CPU and asserted by tests/test_lm_reference_cpu.py: the smallest c with which THIS file's own float64 run stays inside
# (n_act + c) 2^-53 sum|.| of its long-double run, for every entry of H, b and the chi2 of every case of pose_cases(), rounded up to a round figure:
#     python -m tests.test_lm_reference_cpu        ->  largest c over H: 126.7, over b: 578.9, over chi2: 465.8     (x86-64, 80-bit long double)
# rounded up to 600.  The largest figures belong to the cases with ONE active edge: there is no sum to spread the residual's relative error of a few
# hundred 2^-53 (a pixel's difference of coordinates of several hundred) over; from 255 edges on the f64 run needs less than n_act alone.
# The device gets 4 x that, the precedent of ba_reference.C_DEVICE: fused multiply-adds in the sums, one reciprocal where the formulas divide, another
# summation tree.  Nothing here comes from the device's output.
C_F64 = 600
C_DEVICE = 4 * C_F64
ERR_ROUNDINGS = 16     # per residual component: about 16 operations on numbers of pixel-coordinate size (tests/test_ba_one_trial_gpu.py)


def bounds(ref, c):
    """(H, b, chi2) bounds of a long-double linearisation: (n_act + c) 2^-53 x the absolute accumulation"""
    f = (LD(ref["n_act"]) + LD(c)) * LD(U53)
    return f * ref["H_abs"], f * ref["b_abs"], f * ref["chi2"]


def needed_c(ref, H, b, chi2):
    """the c with which the given f64 (H, b, chi2) would just meet bounds(ref, c): one figure each"""
    out = []
    for got, want, acc in ((H, ref["H"], ref["H_abs"]), (b, ref["b"], ref["b_abs"]), (np.array([chi2]), np.array([ref["chi2"]]), np.array([ref["chi2"]]))):
        d = np.abs(np.asarray(got, np.float64).astype(LD) - want)
        ok = acc > 0
        assert np.all(d[~ok] == 0)     # a structural zero (H[3, 4]: d e0 / d ty = d e1 / d tx = 0) must be exactly zero
        out.append(float((d[ok] / (LD(U53) * acc[ok])).max() - ref["n_act"]) if ok.any() else -float(ref["n_act"]))
    return out


def err_bound(ref):
    """per residual component [n_act, 2]: ERR_ROUNDINGS 2^-53 (|obs| + |e| + |principal point|)"""
    return LD(ERR_ROUNDINGS) * LD(U53) * (np.abs(ref["obs"]) + np.abs(ref["e"]) + np.abs(ref["K"][2:4])[None, :])


# ---- the cases of tests/test_poseopt_linearisation_gpu.py (and of the C_F64 measurement) ----------------------------------------------------------------------
POSE_SIZES = (3, 9, 10, 255, 256, 257, 511, 512, 513, 599, 600, 2231, 2232)
PATTERN_SIZES = (513, 600, 2232)
PATTERNS = ("all robust", "all plain", "first of trip off", "second of trip off", "random 30 % off", "only the last")


def pose_problem(n):
    """synth.make_pose_problem without gross outliers and with a small pose error, then 20 % of the observations (at least one) moved by 30 - 60 px in a
    random direction: at the initial pose most edges sit on Huber's quadratic branch and the moved ones on the linear one."""
    from ccm_slam_amd import synth
    p = synth.make_pose_problem(n, 7000 + n, 0.0, pose_sigma_t=0.005, pose_sigma_r_deg=0.1)
    rng = np.random.default_rng(9000 + n)
    moved = rng.permutation(n)[:max(1, int(round(0.2 * n)))]
    ang = rng.uniform(0, 2 * np.pi, moved.size)
    p["obs"] = p["obs"].copy()
    p["obs"][moved] += rng.uniform(30, 60, moved.size)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    p["moved"] = np.sort(moved)
    return p


def pattern_flags(n, pattern):
    """(level, robust) bytes of a named pattern"""
    i = np.arange(n)
    level = np.zeros(n, np.uint8); robust = np.ones(n, np.uint8)
    if pattern == "all plain":
        robust[:] = 0
    elif pattern == "first of trip off":        # a thread's first edge of every trip of 512 inactive, its second active
        level[i % 512 < 256] = 1
    elif pattern == "second of trip off":
        level[i % 512 >= 256] = 1
    elif pattern == "random 30 % off":
        level[np.random.default_rng(11000 + n).random(n) < 0.3] = 1
    elif pattern == "only the last":
        level[:n - 1] = 1
    elif pattern != "all robust":
        raise ValueError(pattern)
    return level, robust


def pose_cases():
    """(n, pattern) of every case"""
    return [(n, pt) for n in POSE_SIZES for pt in (PATTERNS if n in PATTERN_SIZES else PATTERNS[:1])]


# ---- OptimizeSim3 (sim3opt.hip): one linearisation with the reference's numeric Jacobians ---------------------------------------------------------------------
# g2o::Sim3 as ccm_slam_amd/csrc/sim3_math.h states it (sim3.h: the quaternion is not re-normalised by the product or the exponential map); a Sim3 is
# (qx qy qz qw tx ty tz s).  Neither edge overrides linearizeOplus: central differences of the error through the vertex oplus, delta 1e-9
# (base_binary_edge.hpp), the fixed scale applied by zeroing u[6] (VertexSim3Expmap::oplusImpl).
SIM3_DELTA = 1e-9
H7_SLOTS = [(r, c) for r in range(7) for c in range(r, 7)]     # acc[k] = H[r, c]; acc[28 + r] = b[r]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _qrot(q, v, dt):
    """v + w uv + u x uv with uv = 2 (u x v): the rotation by a (unit) quaternion (x, y, z, w) of vectors [..., 3]"""
    uv = dt(2) * _cross(q[:3], v)
    return v + q[3] * uv + _cross(q[:3], uv)


def sim3_exp(u, dt):
    """Sim3(const Vector7d&) (sim3.h:72-140); u = (omega, upsilon, sigma)"""
    u = np.asarray(u, dtype=dt)
    sigma = u[6]
    theta = np.sqrt((u[:3] * u[:3]).sum())
    Om = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]], dtype=dt)
    Om2 = Om @ Om
    I = np.eye(3, dtype=dt)
    s = np.exp(sigma)
    eps = dt(0.00001)
    if theta < eps:
        R = I + Om + Om2
    else:
        R = I + np.sin(theta) / theta * Om + (dt(1) - np.cos(theta)) / (theta * theta) * Om2
    if abs(sigma) < eps:
        C = dt(1)
        if theta < eps:
            A, B = dt(1) / dt(2), dt(1) / dt(6)
        else:
            A = (dt(1) - np.cos(theta)) / (theta * theta)
            B = (theta - np.sin(theta)) / (theta * theta * theta)
    else:
        C = (s - dt(1)) / sigma
        if theta < eps:
            A = ((sigma - dt(1)) * s + dt(1)) / (sigma * sigma)
            B = ((dt(0.5) * sigma * sigma - sigma + dt(1)) * s) / (sigma * sigma * sigma)
        else:
            a, b = s * np.sin(theta), s * np.cos(theta)
            c = theta * theta + sigma * sigma
            A = (a * sigma + (dt(1) - b) * theta) / (theta * c)
            B = (C - ((b - dt(1)) * sigma + a * theta) / c) / (theta * theta)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    assert tr > 0          # (Eigen's Quaterniond(R), trace branch: every rotation met here is a small one)
    t = np.sqrt(tr + dt(1))
    qw = dt(0.5) * t
    t = dt(0.5) / t
    q = np.array([(R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t, qw], dtype=dt)
    W = A * Om + B * Om2 + C * I
    return np.concatenate([q, W @ u[3:6], [s]]).astype(dt)


def sim3_mul(a, b, dt):
    """Sim3::operator* (sim3.h:272-278)"""
    ax, ay, az, aw = a[:4]; bx, by, bz, bw = b[:4]
    q = np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                  aw * bw - ax * bx - ay * by - az * bz], dtype=dt)
    return np.concatenate([q, a[7] * _qrot(a[:4], b[4:7], dt) + a[4:7], [a[7] * b[7]]]).astype(dt)


def sim3_inv(a, dt):
    """Sim3::inverse (sim3.h:240-243)"""
    q = np.array([-a[0], -a[1], -a[2], a[3]], dtype=dt)
    return np.concatenate([q, _qrot(q, (dt(-1) / a[7]) * a[4:7], dt), [dt(1) / a[7]]]).astype(dt)


def sim3_map(S, X, dt):
    """Sim3::map (sim3.h:142-144) of points [n, 3]"""
    return S[7] * _qrot(S[:4], X, dt) + S[4:7]


def _project(S, P, K, dt):
    p = sim3_map(S, P, dt)
    return np.stack([p[:, 0] / p[:, 2] * K[0] + K[2], p[:, 1] / p[:, 2] * K[1] + K[3]], 1)


def sim3_huber_delta(th2):
    """Optimizer.cpp:885: const float deltaHuber = sqrt(th2), th2 a float"""
    return float(np.float32(np.sqrt(np.float32(th2))))


def sim3_perturbed(sim3, fix_scale, dt):
    """[14, 2, 8]: perturbation 2 d / 2 d + 1 = exp(+-delta e_d) * S and its inverse"""
    S = np.asarray(sim3, np.float64).astype(dt)
    out = np.zeros((14, 2, 8), dt)
    for k in range(14):
        u = np.zeros(7, dt)
        u[k // 2] = dt(-SIM3_DELTA) if k & 1 else dt(SIM3_DELTA)
        if fix_scale:
            u[6] = 0
        out[k, 0] = sim3_mul(sim3_exp(u, dt), S, dt)
        out[k, 1] = sim3_inv(out[k, 0], dt)
    return out


def sim3_linearise(p, alive=None, dtype=LD):
    """One linearisation of the problem p (keys of synth.make_sim3_problem) at p["sim3"] over the pairs with alive != 0.

    active   indices of those pairs;  n_act
    proj, e  [n_act, 2 sides, 2]: side 0 is x1 = S X2 under K1 against obs1, side 1 x2 = S^-1 X1 under K2 against obs2
    e2, rho, w   [n_act, 2]
    pert     [14, 2, 8];  J [n_act, 2, 2, 7] (pair, side, row, column) by central differences
    M        [n_act, 2, 2]: |obs| + |projection| + |principal point| of every row
    H [28], b [7] in the kernel's slot order, H_abs, b_abs, chi2 = sum rho
    """
    dt = dtype
    g = lambda k: np.asarray(p[k], np.float64).astype(dt)
    n = np.asarray(p["P1c"]).shape[0]
    act = np.flatnonzero(np.ones(n, np.uint8) if alive is None else np.asarray(alive))
    S = g("sim3")
    P = (g("P2c")[act], g("P1c")[act]); ob = (g("obs1")[act], g("obs2")[act]); K = (g("K1"), g("K2")); om = np.stack([g("info1")[act], g("info2")[act]], 1)
    Sx = (S, sim3_inv(S, dt))
    proj = np.stack([_project(Sx[s], P[s], K[s], dt) for s in (0, 1)], 1)
    obs = np.stack(ob, 1)
    e = obs - proj
    e2 = om * (e * e).sum(2)
    rho, w = huber(e2, np.ones_like(e2, dtype=np.uint8), dt, sim3_huber_delta(p["th2"]))
    pert = sim3_perturbed(p["sim3"], p["fix_scale"], dt)
    J = np.zeros((act.size, 2, 2, 7), dt)
    scalar = dt(1) / (dt(2) * dt(SIM3_DELTA))
    for d in range(7):
        for s in (0, 1):
            ep = ob[s] - _project(pert[2 * d, s], P[s], K[s], dt)
            em = ob[s] - _project(pert[2 * d + 1, s], P[s], K[s], dt)
            J[:, s, :, d] = scalar * (ep - em)
    M = np.abs(obs) + np.abs(proj) + np.stack([np.abs(K[0][2:4]), np.abs(K[1][2:4])])[None]
    out = dict(active=act, n_act=int(act.size), proj=proj, obs=obs, e=e, e2=e2, rho=rho, w=w, info=om, pert=pert, J=J, M=M, chi2=rho.sum())
    out.update(sim3_gather(J, e, om, w, dt))
    return out


def sim3_gather(J, e, om, w, dt=LD):
    """H [28], b [7] and their absolute accumulations from per-pair J [m, 2, 2, 7], e [m, 2, 2], information and Huber weight [m, 2]"""
    J = np.asarray(J).astype(dt); e = np.asarray(e).astype(dt)
    wom = (np.asarray(w).astype(dt) * np.asarray(om).astype(dt))[:, :, None]
    aJ, ae = np.abs(J), np.abs(e)
    return dict(H=np.array([(wom * J[..., r] * J[..., c]).sum() for r, c in H7_SLOTS], dtype=dt),
                H_abs=np.array([(wom * aJ[..., r] * aJ[..., c]).sum() for r, c in H7_SLOTS], dtype=dt),
                b=np.array([-(wom * J[..., r] * e).sum() for r in range(7)], dtype=dt),
                b_abs=np.array([(wom * aJ[..., r] * ae).sum() for r in range(7)], dtype=dt))


def gather_bound(n_act, acc_abs):
    """gamma_m sum|terms|, m = the 4 n_act summed products (2 sides x 2 rows per pair) + 8 for the roundings inside one term"""
    m = LD(4 * n_act + 8) * LD(U53)
    return m / (1 - m) * acc_abs


# C_J: |J_f64 - J_ld| <= C 2^-53 M / (2 delta) — both runs take the same central difference, so its truncation cancels and what is left is the rounding of two
# residuals of size M divided by 2 delta.  MEASURED like C_F64 (python -m tests.test_lm_reference_cpu: the largest C the float64 run needs on sim3_cases());
# the device gets 4 x that.
#     largest C over sim3_cases(): 4.49 (x86-64, 80-bit long double), rounded up to 5
C_J_F64 = 5
C_J = 4 * C_J_F64

SIM3_SIZES = (1, 10, 255, 256, 257, 458, 459, 1136, 1137)     # the staging edges of tests/sim3_opt_cases.py among them
ALIVE_PATTERNS = ("all", "random half", "only the last")


def sim3_problem(n, fix_scale):
    """synth.make_sim3_problem with a fifth of wrong pairs, keyframe 2 under another camera (sim3_opt_cases.two_camera)"""
    from tests import sim3_opt_cases as sc
    from ccm_slam_amd import synth
    p = sc.two_camera(synth.make_sim3_problem(n, 8000 + 2 * n + int(fix_scale), outlier_frac=0.2, fix_scale=fix_scale))
    p["th2"] = 10.0
    return p


def alive_flags(n, pattern):
    alive = np.ones(n, np.uint8)
    if pattern == "random half":
        alive[np.random.default_rng(12000 + n).random(n) < 0.5] = 0
        alive[n - 1] = 1                                  # (never empty)
    elif pattern == "only the last":
        alive[:n - 1] = 0
    elif pattern != "all":
        raise ValueError(pattern)
    return alive


def sim3_cases():
    return [(n, fs, pt) for n in SIM3_SIZES for fs in (False, True) for pt in ALIVE_PATTERNS]
