"""sim3opt.hip: the kernel's FIRST linearisation — chi2, the 14 perturbed estimates, the numeric Jacobians and the accumulated H and b — against long double
(tests/lm_reference.py).  The hook (ccm_debug_sim3opt_linearise) runs the PROBE instantiation of the product kernel: its own staging, chi2_active, perturbation,
accumulation and red.sum64<35>, once, at GIVEN alive flags, in the launch shape the product call takes at that n.

  * every thread holds the same bits of acc[0..34] and of the chi2;
  * H and b equal the long-double gather of the DEVICE's own J and err (Huber weight recomputed in long double from that err) within gamma_m sum|terms|,
    m = the summed products + 8 — whatever is wrong in which pair, side, row or slot a product goes to shows here, free of the Jacobians' own error;
  * J against the long-double central differences: C_J 2^-53 M / (2 delta), M = |obs| + |projection| + |principal point| of the row;
  * a fixed scale: column 6 of J, row and column 6 of H and b[6] are EXACTLY zero;
  * err within 16 roundings of pixel-coordinate size, chi2 within (terms + C_DEVICE) 2^-53 sum rho, pairs that are not alive untouched;
  * the perturbed estimates within 8 x the distance of the reference's own f64 run (floor: 4 ulp of the component's scale).
C_J and C_DEVICE are 4 x what the reference's float64 run needs, measured on the CPU (tests/test_lm_reference_cpu.py)."""
import functools

import numpy as np
import pytest

import sim3_opt_cases as sc
from ccm_slam_amd import optimizer
from tests import lm_reference as lm

LD = np.longdouble
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not lm.HAVE_EXTENDED, reason="numpy.longdouble has no 64-bit mantissa on this platform")]
MARGIN = 8     # tests/test_ba_one_trial_gpu.py: the device may be this many times as far from long double as the reference's own f64 run


@functools.lru_cache(maxsize=None)
def _problem(n, fix_scale):
    return lm.sim3_problem(n, fix_scale)


@functools.lru_cache(maxsize=None)
def _reference(n, fix_scale, pattern, f64):
    r = lm.sim3_linearise(_problem(n, fix_scale), lm.alive_flags(n, pattern), np.float64 if f64 else LD)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _share(d, bound):
    ok = bound > 0
    assert np.all(d[~ok] == 0)
    return float((d[ok] / bound[ok]).max()) if ok.any() else 0.0


def pert_margin(r, f):
    """[14, 2, 8]: MARGIN x the largest distance of the f64 run within the component's group (quaternion, translation, scale; estimate and inverse apart), at
    least 4 ulp of the group's scale (1 for the unit quaternion, the largest |t|, s)"""
    out = np.zeros((14, 2, 8), LD)
    d = np.abs(f["pert"].astype(LD) - r["pert"])
    for side in (0, 1):
        for sl, scale in ((slice(0, 4), LD(1)), (slice(4, 7), np.abs(r["pert"][:, side, 4:7]).max()), (slice(7, 8), np.abs(r["pert"][:, side, 7]).max())):
            out[:, side, sl] = max(MARGIN * d[:, side, sl].max(), 4 * LD(2.0 ** -52) * scale)
    return out


@pytest.mark.parametrize("n,fix_scale,pattern", lm.sim3_cases())
def test_first_linearisation_against_long_double(ctx, n, fix_scale, pattern):
    p = _problem(n, fix_scale)
    alive = lm.alive_flags(n, pattern)
    r = _reference(n, fix_scale, pattern, False)
    d = optimizer.debug_sim3opt_linearise(ctx, *sc.args(p), alive)
    staged = sc.lds_full(n) <= 150 * 1024
    assert (d["use_lds"], d["lds_bytes"]) == (staged, sc.lds_full(n) if staged else sc.LDS_HEAD)
    for name in ("acc", "chi2"):
        bits = np.atleast_2d(d[name]).view(np.uint64)
        same = bits == bits[:, :1]
        assert same.all(), (name, "a thread ended with other bits: (slot, thread)", np.argwhere(~same)[0].tolist())
    H, b, chi2 = d["acc"][:28, 0], d["acc"][28:35, 0], d["chi2"][0]
    act, n_act = r["active"], r["n_act"]
    dead = np.flatnonzero(alive == 0)
    assert not d["err"][dead].any() and not d["J"][dead].any()

    # H and b: the long-double gather of the device's own J and err
    e_dev = d["err"][act].reshape(n_act, 2, 2)
    e2 = r["info"] * (e_dev.astype(LD) ** 2).sum(2)
    _, w = lm.huber(e2, np.ones(e2.shape, np.uint8), LD, lm.sim3_huber_delta(p["th2"]))
    g = lm.sim3_gather(d["J"][act], e_dev, r["info"], w)
    dH, db = np.abs(H.astype(LD) - g["H"]), np.abs(b.astype(LD) - g["b"])
    bH, bb = lm.gather_bound(n_act, g["H_abs"]), lm.gather_bound(n_act, g["b_abs"])

    # J against the long-double central differences
    dJ = np.abs(d["J"][act].astype(LD) - r["J"])
    bJ = LD(lm.C_J) * LD(lm.U53) * r["M"][..., None] / (2 * LD(lm.SIM3_DELTA)) * np.ones((1, 1, 1, 7), LD)

    # err, chi2, perturbed estimates
    de = np.abs(e_dev.astype(LD) - r["e"])
    be = LD(lm.ERR_ROUNDINGS) * LD(lm.U53) * (r["M"] - np.abs(r["proj"]) + np.abs(r["e"]))     # |obs| + |e| + |principal point|
    dc = abs(LD(chi2) - r["chi2"])
    bc = (LD(2 * n_act) + lm.C_DEVICE) * LD(lm.U53) * r["chi2"]
    dp = np.abs(d["pert"].astype(LD) - r["pert"])
    bp = pert_margin(r, _reference(n, fix_scale, pattern, True))
    print(f"n {n} fix_scale {fix_scale} alive {pattern}: n_act {n_act}, share of the bound used: H {_share(dH, bH):.4f}, b {_share(db, bb):.4f}, J {_share(dJ, bJ):.4f}, "
          f"err {_share(de, be):.4f}, chi2 {float(dc / bc):.4f}, pert {_share(dp, bp):.4f}")
    assert np.all(dH <= bH), (int(np.argmax(dH - bH)), _share(dH, bH))
    assert np.all(db <= bb), (int(np.argmax(db - bb)), _share(db, bb))
    assert np.all(dJ <= bJ), _share(dJ, bJ)
    assert np.all(de <= be), _share(de, be)
    assert dc <= bc, float(dc / bc)
    assert np.all(dp <= bp), (np.unravel_index(np.argmax(dp / bp), dp.shape), _share(dp, bp))
    if fix_scale:
        assert not d["J"][..., 6].any()
        assert not np.any(b[6]) and not any(H[k] != 0 for k, (rr, cc) in enumerate(lm.H7_SLOTS) if cc == 6)
        assert np.array_equal(d["pert"][12], d["pert"][13])
