"""poseopt.hip: the kernel's FIRST linearisation, entry by entry against long double (tests/lm_reference.py).

The parity tests of the pose optimiser compare only what ten self-correcting LM iterations end with; a slightly wrong H, a Huber weight on the wrong edge or a
Jacobian column at half strength moves the path, not the fixed point.  The hook (ccm_debug_poseopt_linearise) runs the PROBE instantiation of poseopt_kernel:
the product kernel's own staging and linearise body, once, at GIVEN level / robust flags, in the launch shape the product call takes at that n — and hands back
every thread's reduced acc[0..27] and the err[] array.

Sizes: 3, 9, 10; 255 .. 513 (a thread's first and second edge, trips of 512, the two-edges-per-trip loop with either slot inactive); 599 / 600 (sum28_lds /
sum27); 2231 / 2232 (the last staged size / global memory).  Bounds: (n_act + C_DEVICE) 2^-53 x the absolute accumulation for H, b and the chi2, C_DEVICE = 4 x
what the reference's own float64 run needs (measured on the CPU, tests/test_lm_reference_cpu.py); 16 roundings of pixel-coordinate size per residual.  Each
case prints the share of its bound the device used (DESIGN.md records them beside the bundle adjustment's stage-level bounds)."""
import functools

import numpy as np
import pytest

from ccm_slam_amd import optimizer
from tests import lm_reference as lm

LD = np.longdouble
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not lm.HAVE_EXTENDED, reason="numpy.longdouble has no 64-bit mantissa on this platform")]

# the launch shape poseopt.hip takes (tests/test_poseopt_gpu.py derives the figures): the transpose reduction below 600 edges, its 63 488-byte head beside the
# staged 67 n + 16 bytes; from 600 on the cross-lane reduction with a 4096-byte head; staged in LDS up to 2231 edges
TR_HEAD = (2 * 4 * 64 + 28 * (4 * 64 + 8) + 32) * 8


def expected_shape(n):
    tr = n < 600
    head = TR_HEAD if tr else 4096
    staged = head + 67 * n + 16 <= 150 * 1024
    return dict(tr_red=tr, use_lds=staged, lds_bytes=head + 67 * n + 16 if staged else head)


assert expected_shape(599)["lds_bytes"] == 63488 + 67 * 599 + 16 and not expected_shape(2232)["use_lds"] and expected_shape(2231)["use_lds"]


@functools.lru_cache(maxsize=None)
def _problem(n):
    return lm.pose_problem(n)


@functools.lru_cache(maxsize=None)
def _reference(n, pattern):
    p = _problem(n)
    level, robust = lm.pattern_flags(n, pattern)
    r = lm.pose_linearise(p["cam_qt"], p["Xw"], p["obs"], p["info"], p["K"], level, robust)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _share(d, bound):
    """largest d / bound over the entries with a positive bound"""
    ok = bound > 0
    return float((d[ok] / bound[ok]).max())


@pytest.mark.parametrize("n,pattern", lm.pose_cases())
def test_first_linearisation_against_long_double(ctx, n, pattern):
    p = _problem(n)
    level, robust = lm.pattern_flags(n, pattern)
    r = _reference(n, pattern)
    d = optimizer.debug_poseopt_linearise(ctx, p["cam_qt"], p["Xw"], p["obs"], p["info"], p["K"], level, robust)
    assert {k: d[k] for k in ("tr_red", "use_lds", "lds_bytes")} == expected_shape(n)
    acc = d["acc"]
    bits = acc.view(np.uint64)
    same = bits == bits[:, :1]
    assert same.all(), ("a thread ended with other bits: (slot, thread)", np.argwhere(~same)[0].tolist())
    H, b, chi2 = acc[:21, 0], acc[21:27, 0], acc[27, 0]
    bH, bb, bc = lm.bounds(r, lm.C_DEVICE)
    dH, db, dc = np.abs(H.astype(LD) - r["H"]), np.abs(b.astype(LD) - r["b"]), abs(LD(chi2) - r["chi2"])
    # residuals: active edges within 16 roundings of pixel-coordinate size, inactive ones as the kernel initialised them
    de = np.abs(d["err"][r["active"]].astype(LD) - r["e"])
    be = lm.err_bound(r)
    print(f"n {n} {pattern}: n_act {r['n_act']}, share of the bound used: H {_share(dH, bH):.4f}, b {_share(db, bb):.4f}, chi2 {float(dc / bc):.4f}, "
          f"err {_share(de, be):.4f}")
    assert np.all(dH <= bH), (int(np.argmax(dH - bH)), _share(dH, bH))     # (H[3, 4] is a structural zero: its bound is 0 and so must the entry be)
    assert np.all(db <= bb), (int(np.argmax(db - bb)), _share(db, bb))
    assert dc <= bc, float(dc / bc)
    assert np.all(de <= be), _share(de, be)
    z = lm.H_SLOTS.index((3, 4))
    assert bH[z] == 0 and H[z] == 0 and (np.delete(bH, z) > 0).all()
    inactive = np.flatnonzero(level != 0)
    assert np.array_equal(d["err"][inactive].view(np.uint64), np.zeros((inactive.size, 2), np.uint64))
