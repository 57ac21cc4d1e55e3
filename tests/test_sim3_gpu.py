"""Optimizer::OptimizeSim3 on the device vs the oracle restatement (oracle/ba_ref.cpp: ora_sim3_optimize).

Observables: the inlier flags and the inlier count (identical, always) and the optimised Sim3.  Both sides are f64 Levenberg-Marquardt with numerically
differentiated Jacobians (delta 1e-9, which amplifies every rounding by 5e8); the device sums H in a different association order, contracts to FMAs where the
oracle's plain build does not, and uses the device libm.  The first seven tests allow 1e-6 on quaternion / scale and 1e-6 m on translation.  That figure is not
"~1e-9" of headroom: the reference's own resolution, measured by tests/test_sim3_threshold_cpu.py (plain oracle build against the -O3 -march=native build of the
same source, on the 168 problems of sim3_opt_cases.sweep_cases() as generated and with a residual planted at the chi2 threshold), is

  estimate, identical flags and nIn >= 16:  1.01e-5 at most (one problem of 700 pairs planted at 1e-4 / 1e-5; 4.2e-7 over all other cases; below 16 inliers the
      estimate amplifies rounding and is not compared)                         => every new test here allows EST_TOL = 4 x 1.01e-5 (three rounding-level
      departures of the device against one between the builds)
  flags / nIn, planted at relative delta from the oracle's flip:  the builds differ in 0 / 0 / 1 / 17 / 99 of 302 calls at 1e-4 / 1e-5 / 1e-6 / 1e-7 / 1e-8
      (0.33 % at 1e-6, 5.6 % at 1e-7)                                          => identical at 1e-4 and 1e-5; counted at 1e-6 / 1e-7 against twice these shares
      (1 % floor at 1e-6).  The device (MI355X): 1 and 20 of 302 (0.33 %, 6.6 %; DEVICE_SHARES), largest estimate difference over the sweep's 772
      must-calls 1.00e-5.  On another CPU model the -march=native build gives 0 / 0 / 1 / 23 / 94 and 1.02e-5.

Launch shapes (ccm_sim3_optimize; derivation in sim3_opt_cases.py): dynamic LDS = 5904 + 130 n bytes (512 reduction + 224 perturbation doubles, 16 doubles + 2 flag
bytes per pair, + 16): n <= 458 fits 64 KiB; 459 <= n <= 1136 raises the kernel's dynamic-LDS limit to 150 KiB and stages everything; n >= 1137 keeps the problem
in global memory.

The flags are decided from the errors of the last EVALUATED LM trial, which may be a rejected one (the kernel's over() reads a.err; ba_ref.cpp, note in
ora_pose_optimize, for the same g2o behaviour): no test here recomputes chi2 at the returned estimate.
"""
import numpy as np
import pytest

import sim3_opt_cases as sc
from ccm_slam_amd import optimizer, synth

pytestmark = pytest.mark.gpu

# share of the calls planted at 1e-6 / 1e-7 on which the device differs from the plain oracle, measured by the sweep below on an MI355X (the reference's own builds:
# sc.REF_SHARE); asserted against sc.share_cap, recorded here
DEVICE_SHARES = {1e-6: 1 / 302, 1e-7: 20 / 302}     # 0.33 % and 6.6 %; caps 1 % and 11.3 %


def _run_both(ctx, p):
    import oracle
    args = (p["sim3"], p["P1c"], p["P2c"], p["obs1"], p["obs2"], p["info1"], p["info2"], p["K1"], p["K2"], p["th2"], p["fix_scale"])
    return optimizer.sim3_optimization(ctx, *args), oracle.sim3_optimize(*args)


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("seed,n", [(0, 150), (1, 60), (2, 400), (3, 23)])
def test_sim3_matches_oracle(ctx, oracle_lib, seed, n, fix_scale):
    p = synth.make_sim3_problem(n, seed, fix_scale=fix_scale)
    (s, inl, nin), (so, inlo, nino) = _run_both(ctx, p)
    assert nin == nino and nin > 0
    assert np.array_equal(inl, inlo)
    assert np.abs(s - so).max() < 1e-6, np.abs(s - so)
    if fix_scale:
        assert s[7] == p["sim3"][7]
    # and it actually optimised: closer to the truth than the start, gross outliers rejected
    assert np.abs(s[4:7] - p["gt_sim3"][4:7]).max() < np.abs(p["sim3"][4:7] - p["gt_sim3"][4:7]).max()
    assert (inl[p["is_outlier"]] == 0).mean() > 0.9


def test_fewer_than_ten_survivors_returns_zero_and_keeps_input(ctx, oracle_lib):
    p = synth.make_sim3_problem(9, 5)
    (s, inl, nin), (so, inlo, nino) = _run_both(ctx, p)
    assert nin == 0 and nino == 0
    assert np.array_equal(s, p["sim3"]) and np.array_equal(so, p["sim3"])
    assert np.array_equal(inl, inlo)


def test_mostly_outliers_returns_zero(ctx, oracle_lib):
    p = synth.make_sim3_problem(30, 6, outlier_frac=0.8)
    (s, inl, nin), (so, inlo, nino) = _run_both(ctx, p)
    assert nin == nino
    assert np.array_equal(inl, inlo)
    if nin == 0:
        assert np.array_equal(s, p["sim3"])


def test_empty_input(ctx):
    z = np.zeros((0, 3)); z2 = np.zeros((0, 2)); z1 = np.zeros(0)
    s0 = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
    s, inl, nin = optimizer.sim3_optimization(ctx, s0, z, z, z2, z2, z1, z1, synth.EUROC_K, synth.EUROC_K)
    assert nin == 0 and np.array_equal(s, s0) and inl.size == 0


def test_large_problem_uses_global_memory_path(ctx, oracle_lib):
    p = synth.make_sim3_problem(1500, 7)     # 16 doubles/pair > the 150 KB LDS budget
    (s, inl, nin), (so, inlo, nino) = _run_both(ctx, p)
    assert nin == nino and np.array_equal(inl, inlo)
    assert np.abs(s - so).max() < 1e-6


# ---- two cameras, outliers on either side, th2, fixed scales other than 1, launch shapes, the survivor gate, residuals planted at the threshold --------------------
# (problems: tests/sim3_opt_cases.py; tolerances: the module docstring)

def _same_as_oracle(ctx, oracle_lib, p, what=""):
    """device against oracle on one problem: identical flags and count, estimate within sc.EST_TOL where the oracle counts >= 16 inliers"""
    got = optimizer.sim3_optimization(ctx, *sc.args(p))
    want = oracle_lib.sim3_optimize(*sc.args(p))
    assert got[2] == want[2] and np.array_equal(got[1], want[1]), (what, got[2], want[2], np.flatnonzero(got[1] != want[1]))
    if want[2] >= sc.MIN_INLIERS_FOR_ESTIMATE:
        _worst[0] = max(_worst[0], float(np.abs(got[0] - want[0]).max()))
        assert np.abs(got[0] - want[0]).max() <= sc.EST_TOL, (what, np.abs(got[0] - want[0]))
    return got, want


_worst = [0.0]   # largest estimate difference seen by _same_as_oracle (printed by the sweep; the bound is sc.EST_TOL, from the CPU)


@pytest.mark.parametrize("sides", [(1, 0), (0, 1), (1, 1)], ids=["obs1", "obs2", "both"])
@pytest.mark.parametrize("n", [23, 150])
@pytest.mark.parametrize("th2", [7.0, 10.0, 16.0])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_two_cameras_outliers_on_either_side(ctx, oracle_lib, fix_scale, th2, n, sides):
    n_out = max(2, n // 10)
    for scale in ((0.8, 1.2) if fix_scale else (None,)):
        p, i0, i1 = sc.two_sided(n, 300 + n, n_out * sides[0], n_out * sides[1], fix_scale=fix_scale, th2=th2, scale=scale)
        assert not np.array_equal(p["K1"], p["K2"])
        (s, inl, nin), _ = _same_as_oracle(ctx, oracle_lib, p, (scale,))
        assert nin > 0 and not np.array_equal(s, p["sim3"])
        assert (inl[np.concatenate([i0, i1])] == 0).all()      # every gross outlier is rejected, whichever edge sees it
        if fix_scale:
            assert p["sim3"][7] == scale and s[7] == p["sim3"][7]     # bit-equal: the scale is never touched


def test_exchanged_cameras_follow_the_oracle_and_are_visible(ctx, oracle_lib):
    p, _, _ = sc.two_sided(150, 450, 15, 15)
    x = dict(p, K1=p["K2"], K2=p["K1"])
    _, want = _same_as_oracle(ctx, oracle_lib, p)
    _, want_x = _same_as_oracle(ctx, oracle_lib, x, "K1 <-> K2")
    # the case can see an exchange: the oracle itself answers differently
    assert want_x[2] != want[2] and not np.array_equal(want_x[1], want[1]) and np.abs(want_x[0] - want[0]).max() > 1e-2


def _staging_problem(n, fix_scale=False):
    n_out = n // 10
    return sc.two_sided(n, 300 + n, n_out, n_out, fix_scale=fix_scale, scale=1.2 if fix_scale else None)[0]


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("n", sc.STAGING_EDGES)
def test_staging_boundaries(ctx, oracle_lib, n, fix_scale):
    # lds_full = (kRedDoubles 512 + kPertDoubles 224) * 8 + (16 * 8 + 2) n + 16 = 5904 + 130 n (ccm_sim3_optimize): 458 is the last n under 64 KiB, 1136 the last under
    # 150 KiB; a change of kRedDoubles / kPertDoubles or of the per-pair layout moves these and must move sc.LDS_HEAD / sc.LDS_PER_PAIR with it
    assert sc.STAGING_EDGES == (458, 459, 1136, 1137)
    assert sc.lds_full(1136) == 5904 + 130 * 1136
    assert 5904 + 130 * 458 <= 64 * 1024 < 5904 + 130 * 459
    assert 5904 + 130 * 1136 <= 150 * 1024 < 5904 + 130 * 1137
    p = _staging_problem(n, fix_scale)
    (s, inl, nin), _ = _same_as_oracle(ctx, oracle_lib, p)
    assert nin >= 0.7 * n
    if fix_scale:
        assert s[7] == 1.2


def test_fresh_context_starts_with_the_largest_lds_launch(oracle_lib):
    """the raised dynamic-LDS limit on a context that has not set it yet, then a small launch and the global-memory launch on the same context"""
    from ccm_slam_amd._lib import Context
    c = Context(0)
    try:
        for n in (1136, 23, 1137):
            _same_as_oracle(c, oracle_lib, _staging_problem(n), n)
    finally:
        c.close()


def test_largest_lds_launch_is_deterministic(ctx):
    p = _staging_problem(1136)
    a = optimizer.sim3_optimization(ctx, *sc.args(p))
    b = optimizer.sim3_optimization(ctx, *sc.args(p))
    assert a[2] == b[2] > 0 and np.array_equal(a[1], b[1])
    assert a[0].tobytes() == b[0].tobytes()        # block reductions in a fixed order: bit-identical


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("n,n_out", [(14, 4), (14, 5), (30, 20), (30, 21), (10, 0), (10, 1)])
def test_survivor_gate_at_ten_against_nine(ctx, oracle_lib, n, n_out, side):
    p, idx = sc.survivor_case(oracle_lib, n, n_out, side)
    (s, inl, nin), _ = _same_as_oracle(ctx, oracle_lib, p)
    assert np.array_equal(np.flatnonzero(inl == 0), np.sort(idx))       # the first pass's drops stay visible either way
    if n - n_out == 10:
        assert nin == 10 and not np.array_equal(s, p["sim3"])
    else:
        assert n - n_out == 9 and nin == 0 and s.tobytes() == np.ascontiguousarray(p["sim3"], np.float64).tobytes()


def test_sweep_with_residuals_planted_at_the_threshold(ctx, oracle_lib):
    """sc.sweep_cases(): 168 problems of 10 .. 700 pairs (two cameras, 0 / 10 / 30 % gross outliers split between the sides, th2 7 / 10 / 16, free and fixed scale) as
    generated, and each one on which plant_at_threshold succeeds again with the planted pair's residual at lo (1 - delta) and hi (1 + delta) of the oracle's flip.
    delta 1e-4, 1e-5: flags and nIn identical, estimate within EST_TOL where nIn >= 16.  delta 1e-6, 1e-7: counted — the device may differ from the plain oracle
    in at most twice the share of calls in which the oracle's -O3 -march=native build does (1 / 302 and 17 / 302; 1 % floor at 1e-6), and only starting from the
    planted pair's flag.  Measured on the device: see DEVICE_SHARES."""
    n_must = n_planted = 0
    _worst[0] = 0.0
    calls = {d: 0 for d in sc.COUNTED_DELTAS}
    diff = {d: 0 for d in sc.COUNTED_DELTAS}
    wider = 0
    for case, p, j, pl in sc.sweep(oracle_lib):
        _same_as_oracle(ctx, oracle_lib, p, ("as generated", case))
        n_must += 1
        if pl is None:
            continue
        n_planted += 1
        for d, q in sc.sweep_variants(p, j, case[4], pl, sc.MUST_DELTAS):
            _same_as_oracle(ctx, oracle_lib, q, (d, case, j))
            n_must += 1
        for d, q in sc.sweep_variants(p, j, case[4], pl, sc.COUNTED_DELTAS):
            got = optimizer.sim3_optimization(ctx, *sc.args(q))
            want = oracle_lib.sim3_optimize(*sc.args(q))
            calls[d] += 1
            if got[2] != want[2] or not np.array_equal(got[1], want[1]):
                diff[d] += 1
                assert sc.planted_pair_differs(j, got, want), (d, case, j, np.flatnonzero(got[1] != want[1]), got[2], want[2])
                wider += 0 if sc.only_planted_pair(j, got, want) else 1
    print(f"sim3 sweep: {n_planted} planted, {n_must} must-calls, device differs in {diff} of {calls} ({wider} in more than the planted pair); "
          f"largest estimate difference over the must-calls with nIn >= 16: {_worst[0]:.3e}")
    assert n_planted >= 120 and n_must >= 400, (n_planted, n_must)
    for d in sc.COUNTED_DELTAS:
        assert diff[d] <= sc.share_cap(d) * calls[d], (d, diff, calls)
