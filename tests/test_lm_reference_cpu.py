"""CPU: tests/lm_reference.py pinned independently of the device.

  * its rotation, Huber and Jacobian formulas reproduce those of tests/ba_reference.py exactly in long double;
  * b = -1/2 x the central-difference gradient (long double) of its own robust chi2 with respect to the left-multiplied se(3) increment in g2o's order
    (omega, upsilon): signs and slot order of b, and through the LM loop below those of H;
  * a plain LM loop on its H and b, on a problem without outliers, ends within 1e-7 of oracle.pose_optimize (the project's bar for that pose);
  * C_F64 is what its own float64 run needs on the cases of the GPU test, and the bounds with C_DEVICE = 4 C_F64 reject three mutations of that f64 run.

  * the Sim3 side: exp / inverse / product / map obey the group laws and reduce to SE3Quat::exp without scale; b = -1/2 the gradient of the robust chi2 through
    the vertex oplus (fixed scale included); C_J is what the float64 run's numeric Jacobians need; an f64 gather in numpy's order meets the gather bound.

`python -m tests.test_lm_reference_cpu` prints the measurements behind C_F64 and C_J."""
import numpy as np
import pytest

from tests import ba_reference as ref
from tests import lm_reference as lm

LD = np.longdouble
pytestmark = pytest.mark.skipif(not lm.HAVE_EXTENDED, reason="numpy.longdouble has no 64-bit mantissa on this platform")


def _lin(p, level=None, robust=None, dtype=LD, cam=None):
    return lm.pose_linearise(p["cam_qt"] if cam is None else cam, p["Xw"], p["obs"], p["info"], p["K"], level, robust, dtype)


def test_the_formulas_are_those_of_the_ba_reference():
    p = lm.pose_problem(257)
    r = _lin(p)
    R = ref.rot_from_quat(ref._ld(p["cam_qt"])[None, :4])
    assert np.array_equal(lm.rot(ref._ld(p["cam_qt"])[:4], LD), R[0])
    _, Jj = ref.jacobians(r["Xc"], np.repeat(R, 257, 0), np.tile(ref._ld(p["K"]), (257, 1)))
    assert np.array_equal(r["J"], Jj)
    rho0, rho1 = ref.huber(r["e2"], lm.HUBER_DELTA)
    assert np.array_equal(r["rho"], rho0) and np.array_equal(r["w"], rho1)
    assert (r["w"] < 1).any() and (r["w"] == 1).any()
    plain = _lin(p, robust=np.zeros(257, np.uint8))
    assert np.array_equal(plain["rho"], plain["e2"]) and (plain["w"] == 1).all()
    assert lm.HUBER_DELTA == float(np.float32(np.sqrt(5.991)))


@pytest.mark.parametrize("n,pattern", [(10, "all robust"), (513, "random 30 % off"), (600, "all plain")])
def test_b_is_minus_half_the_gradient_of_the_robust_chi2(n, pattern):
    p = lm.pose_problem(n)
    level, robust = lm.pattern_flags(n, pattern)
    r = _lin(p, level, robust)
    h = LD(1e-6)
    g = np.zeros(6, LD)
    for k in range(6):
        u = np.zeros(6, LD); u[k] = h
        g[k] = (_lin(p, level, robust, cam=ref.oplus(u, p["cam_qt"]))["chi2"] - _lin(p, level, robust, cam=ref.oplus(-u, p["cam_qt"]))["chi2"]) / (2 * h)
    # truncation of the central difference: h^2 x a third derivative, far below 1e-7 of the accumulation of b
    assert np.all(np.abs(r["b"] + g / 2) <= LD(1e-7) * r["b_abs"]), (np.abs(r["b"] + g / 2) / r["b_abs"]).astype(float)
    assert np.all(np.abs(r["b"]) > LD(1e-3) * r["b_abs"])     # no entry of b is so small that its sign would go unnoticed
    # H is symmetric positive definite in its slot order, and the Gauss-Newton step on (H, b) lowers the chi2
    H = lm.full_H(r["H"])
    assert np.all(np.linalg.eigvalsh(H.astype(np.float64)) > 0)
    x = ref.solve_refined(H, r["b"])
    assert _lin(p, level, robust, cam=ref.oplus(x, p["cam_qt"]))["chi2"] < r["chi2"]


def _clean_problem(n, seed):
    """make_pose_problem without outliers and with the observation noise shrunk to 0.3 of itself: no edge comes near chi2 = 5.991 at the optimum, so every
    round of the schedule optimises all edges on Huber's quadratic branch and a plain LM loop has the same fixed point"""
    from ccm_slam_amd import synth
    p = synth.make_pose_problem(n, seed, 0.0)
    gt = p["gt_cam_qt"]
    R = np.asarray(lm.rot(gt[:4], np.float64))
    Xc = p["Xw"] @ R.T + gt[4:]
    proj = np.stack([p["K"][0] * Xc[:, 0] / Xc[:, 2] + p["K"][2], p["K"][1] * Xc[:, 1] / Xc[:, 2] + p["K"][3]], 1)
    p["obs"] = proj + 0.3 * (p["obs"] - proj)
    return p


@pytest.mark.parametrize("n,seed", [(40, 21), (300, 22)])
def test_plain_lm_on_the_reference_ends_at_the_oracles_pose(oracle_lib, n, seed):
    p = _clean_problem(n, seed)
    ocam, ooutl, oninl = oracle_lib.pose_optimize(p["cam_qt"], p["Xw"], p["obs"], p["info"], p["K"])
    assert oninl == n and not ooutl.any()
    cam = ref._ld(p["cam_qt"])
    r = _lin(p, cam=cam)
    lam = LD(1e-5) * np.abs(np.diag(lm.full_H(r["H"]))).max()
    for _ in range(30):
        x = ref.solve_refined(lm.full_H(r["H"]) + lam * np.eye(6, dtype=LD), r["b"])
        trial = ref.oplus(x, cam)
        rt = _lin(p, cam=trial)
        if rt["chi2"] < r["chi2"]:
            cam, r, lam = trial, rt, lam / 3
        else:
            lam *= 4
        if np.abs(x).max() < 1e-14:
            break
    assert (r["e2"] < 5.991 / 2).all()
    got = cam.astype(np.float64)
    if got[3] * ocam[3] < 0:
        got[:4] = -got[:4]
    assert np.abs(got - ocam).max() < 1e-7, np.abs(got - ocam).max()


def _measure():
    worst = np.full(3, -np.inf)
    rows = []
    for n, pattern in lm.pose_cases():
        p = lm.pose_problem(n)
        level, robust = lm.pattern_flags(n, pattern)
        r = _lin(p, level, robust)
        f = _lin(p, level, robust, dtype=np.float64)
        c = np.array(lm.needed_c(r, f["H"], f["b"], f["chi2"]))
        rows.append((n, pattern, r["n_act"], int((r["w"] < 1).sum()), c))
        worst = np.maximum(worst, c)
    return rows, worst


def test_c_f64_is_what_the_float64_run_needs():
    rows, worst = _measure()
    assert len(rows) == 13 + 3 * 5
    assert worst.max() <= lm.C_F64, worst              # the f64 run meets the bound with C_F64 on every case ...
    assert worst.max() > lm.C_F64 / 2, worst           # ... and C_F64 is that figure rounded up, not a generous one
    assert lm.C_DEVICE == 4 * lm.C_F64
    for n, pattern, n_act, n_lin, _ in rows:           # both Huber branches occur wherever there is room for them
        if n_act >= 9 and pattern != "all plain":
            assert 0 < n_lin < n_act, (n, pattern, n_lin)


def _inside(r, H, b, chi2):
    bH, bb, bc = lm.bounds(r, lm.C_DEVICE)
    return bool(np.all(np.abs(H.astype(LD) - r["H"]) <= bH) and np.all(np.abs(b.astype(LD) - r["b"]) <= bb) and abs(LD(chi2) - r["chi2"]) <= bc)


def test_the_bounds_reject_a_missing_edge_swapped_slots_and_a_lost_huber_weight():
    n = 2232
    p = lm.pose_problem(n)
    r = _lin(p)
    f = _lin(p, dtype=np.float64)
    assert _inside(r, f["H"], f["b"], f["chi2"])
    # one edge's contribution removed (an inlier of ordinary size: the smallest change such a defect can make is one term of 2232)
    k = int(np.flatnonzero(f["w"] == 1)[n // 2])
    level = np.zeros(n, np.uint8); level[k] = 1
    m = _lin(p, level, dtype=np.float64)
    assert not _inside(r, m["H"], f["b"], f["chi2"])
    assert not _inside(r, f["H"], m["b"], f["chi2"])
    assert not _inside(r, f["H"], f["b"], m["chi2"])
    # two H slots exchanged
    for s, t in ((0, 1), (7, 8), (19, 20), (3, 15)):
        H = f["H"].copy(); H[[s, t]] = H[[t, s]]
        assert not _inside(r, H, f["b"], f["chi2"]), (s, t)
    # one outlier's Huber weight set to 1: its edge enters H and b with w = 1 and the chi2 with rho = e2
    k = int(np.flatnonzero(f["w"] < 1)[0])
    robust = np.ones(n, np.uint8); robust[k] = 0
    m = _lin(p, None, robust, dtype=np.float64)
    assert not _inside(r, m["H"], f["b"], f["chi2"])
    assert not _inside(r, f["H"], m["b"], f["chi2"])
    assert not _inside(r, f["H"], f["b"], m["chi2"])


# ---- the Sim3 side --------------------------------------------------------------------------------------------------------------------------------------------

def test_sim3_algebra_as_sim3_math_states_it():
    rng = np.random.default_rng(5)
    for _ in range(4):
        u = np.concatenate([rng.normal(size=3) * 0.3, rng.normal(size=3), [rng.normal() * 0.2]])
        S = lm.sim3_exp(u, LD)
        assert abs(S[7] - np.exp(LD(u[6]))) < 1e-18 and abs((S[:4] ** 2).sum() - 1) < 1e-17
        E = lm.sim3_mul(S, lm.sim3_inv(S, LD), LD)
        assert np.abs(E - np.array([0, 0, 0, 1, 0, 0, 0, 1], LD)).max() < 1e-17
        X = rng.normal(size=(5, 3)).astype(LD)
        assert np.abs(lm.sim3_map(lm.sim3_inv(S, LD), lm.sim3_map(S, X, LD), LD) - X).max() < 1e-17
        # a product maps like the two maps in turn; without scale the exponential is SE3Quat::exp
        T = lm.sim3_exp(u[::-1].copy() * 0.5, LD)
        assert np.abs(lm.sim3_map(lm.sim3_mul(S, T, LD), X, LD) - lm.sim3_map(S, lm.sim3_map(T, X, LD), LD)).max() < 1e-17
        u0 = u.copy(); u0[6] = 0
        q, t = ref.se3_exp(u0[:6])
        S0 = lm.sim3_exp(u0, LD)
        assert np.abs(S0[:4] - q).max() < 1e-17 and np.abs(S0[4:7] - t).max() < 1e-17 and S0[7] == 1
    # one-parameter subgroup: exp(2 u) = exp(u) exp(u) — pins the translation coefficients A, B, C with scale and rotation both present
    u = np.array([0.1, -0.2, 0.15, 0.3, -0.1, 0.2, 0.12])
    a, b2 = lm.sim3_exp(2 * u, LD), lm.sim3_mul(lm.sim3_exp(u, LD), lm.sim3_exp(u, LD), LD)
    assert np.abs(a - b2).max() < 1e-17


@pytest.mark.parametrize("n,fix_scale,pattern", [(10, False, "all"), (257, True, "random half"), (257, False, "all")])
def test_sim3_b_is_minus_half_the_gradient_of_the_robust_chi2(n, fix_scale, pattern):
    p = lm.sim3_problem(n, fix_scale)
    alive = lm.alive_flags(n, pattern)
    r = lm.sim3_linearise(p, alive)
    h = LD(1e-6)
    g = np.zeros(7, LD)
    S = ref._ld(p["sim3"])
    for k in range(7):
        u = np.zeros(7, LD); u[k] = h
        if fix_scale:
            u[6] = 0
        cp = lm.sim3_linearise(dict(p, sim3=lm.sim3_mul(lm.sim3_exp(u, LD), S, LD)), alive)["chi2"]
        cm = lm.sim3_linearise(dict(p, sim3=lm.sim3_mul(lm.sim3_exp(-u, LD), S, LD)), alive)["chi2"]
        g[k] = (cp - cm) / (2 * h)
    assert np.all(np.abs(r["b"] + g / 2) <= LD(1e-6) * np.maximum(r["b_abs"], 1e-300)), (np.abs(r["b"] + g / 2) / r["b_abs"]).astype(float)
    if fix_scale:
        assert r["b"][6] == 0 and not r["J"][..., 6].any()


def _measure_sim3():
    worst_j = worst_c = worst_g = 0.0
    for n, fs, pattern in lm.sim3_cases():
        p = lm.sim3_problem(n, fs)
        alive = lm.alive_flags(n, pattern)
        r = lm.sim3_linearise(p, alive)
        f = lm.sim3_linearise(p, alive, np.float64)
        worst_j = max(worst_j, float((np.abs(f["J"].astype(LD) - r["J"]) / (LD(lm.U53) * r["M"][..., None] / (2 * LD(lm.SIM3_DELTA)))).max()))
        worst_c = max(worst_c, float(abs(LD(f["chi2"]) - r["chi2"]) / (LD(lm.U53) * r["chi2"])) - 2 * r["n_act"])
        # the f64 gather of the f64 run's J and err, numpy's pairwise order, against the long-double gather of the same J and err
        g = lm.sim3_gather(f["J"], f["e"], f["info"], f["w"], LD)
        g64 = lm.sim3_gather(f["J"], f["e"], f["info"], f["w"], np.float64)
        for k in ("H", "b"):
            d, bd = np.abs(g64[k].astype(LD) - g[k]), lm.gather_bound(r["n_act"], g[k + "_abs"])
            assert np.all(d[bd == 0] == 0)
            worst_g = max(worst_g, float((d[bd > 0] / bd[bd > 0]).max()))
        assert (r["w"] < 1).any() or r["n_act"] == 1
    return worst_j, worst_c, worst_g


def test_c_j_is_what_the_float64_run_needs_and_an_f64_gather_meets_its_bound():
    worst_j, worst_c, worst_g = _measure_sim3()
    assert lm.C_J_F64 / 2 < worst_j <= lm.C_J_F64 and lm.C_J == 4 * lm.C_J_F64, worst_j
    assert worst_c <= lm.C_F64, worst_c              # the chi2 of the Sim3 edges needs no more than the pose edges' constant
    assert worst_g <= 1.0, worst_g


if __name__ == "__main__":
    rows, worst = _measure()
    for n, pattern, n_act, n_lin, c in rows:
        print(f"n {n:5d} {pattern:20s} active {n_act:5d} on Huber's linear branch {n_lin:4d}   c needed: H {c[0]:8.1f}  b {c[1]:8.1f}  chi2 {c[2]:8.1f}")
    print(f"largest c over H: {worst[0]:.1f}, over b: {worst[1]:.1f}, over chi2: {worst[2]:.1f}")
    print("Sim3: largest C_J of the f64 run %.2f, largest c of its chi2 %.1f, largest share of the gather bound an f64 gather uses %.3f" % _measure_sim3())
