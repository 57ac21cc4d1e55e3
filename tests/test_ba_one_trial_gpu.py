"""One complete LM trial on the device (h.run(1, lambda_init=...): linearise, D^-1, Schur, the reduced solve, ba_update_cams, back-substitution +
chi2, ba_reduce_scalars) against the long-double reference step of tests/ba_reference.py.

Exact reduced solves (ba_solve_cholreg, ba_solve_dense2): the same step taken by the f64 oracle (ba_optimize(prob, 1, linear_solver=1, lambda_init=...),
not the code under test) is measured against the reference in the test itself, per quantity; the device is allowed 8 x that distance (two different
factorisations and summation orders; f32 appears nowhere on this path).  Only the next lambda has a floor: its oracle distance is exactly 0 wherever
the gain ratio clips the factor to 1/3.  chi2_initial involves no solve and is held to the accumulation bound (n = active edges).

PCG-solved maps (ba_pcg_small, ba_pcg_persist, the multi-kernel PCG): the camera step, recovered from the downloaded poses by the long-double log map,
is judged as a residual, |(S_ref + lambda I) dx_dev - b_ref| <= 2 rel_tol |b_ref|; the landmark step against D^-1 (b_l - W^T dx_dev) at the accumulation
bound; chi2 and the per-edge chi2 against the reference AT the downloaded state.

Every case asserts which solver it reached: the launch counts of the two solver profiling scopes, `pers_grid` of the handle, and the solver's own
iteration count (the exact solvers report exactly one per trial).  Measured oracle distances: tests/test_ba_reference_cpu.py, DESIGN.md section 3."""
import numpy as np
import pytest

import oracle
from ccm_slam_amd import optimizer, synth
from ccm_slam_amd._lib import K
from tests import ba_reference as ref
from tests.test_ba_reduced_system_gpu import _one_long_track

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.HAVE_EXTENDED, reason="numpy.longdouble has no 64-bit mantissa on this platform")]
LD = ref.LD
MARGIN = 8
LAM_NEXT_FLOOR = 16 * ref.U53     # the oracle's next lambda equals the reference's bit for bit where the factor is clipped to 1/3: 8 x 0 would allow nothing


def _distances(cam, pts, chi2_edge, dpos, chi2_final, lam_after, stp, lam_next):
    dc, dr = ref.pose_distance(cam, stp["cam"])
    act = stp["edges"]
    return dict(centre=float(dc.max()), rot=float(dr.max()), pts=float(np.abs(pts.astype(LD) - stp["pts"]).max()),
                edge_chi2=float((np.abs(chi2_edge[act].astype(LD) - stp["edge_chi2"]) / np.maximum(stp["edge_chi2"], 1)).max()),
                chi2_final=float(abs(LD(chi2_final) - stp["chi2"]) / stp["chi2"]),
                lam_next=float(abs(LD(lam_after) - lam_next) / lam_next)), bool(np.array_equal(dpos[act] != 0, stp["depth_pos"]))


def _allowed(d_or):
    return {k: MARGIN * (max(v, LAM_NEXT_FLOOR) if k == "lam_next" else v) for k, v in d_or.items()}


def _run(ctx, h, iters, lam, **kw):
    """(stats, launches of the CCM_K_BA_PCG_PERSIST scope, launches of the CCM_K_BA_PCG_SPMV scope) of one run"""
    ctx.prof_enable(-1); ctx.prof_reset()
    st = h.run(iters, lambda_init=lam, **kw)
    n_pers, _ = ctx.prof_read(K["BA_PCG_PERSIST"])
    n_spmv, _ = ctx.prof_read(K["BA_PCG_SPMV"])
    ctx.prof_enable(-2)
    return st, n_pers, n_spmv


def _assert_solver(solver, sz, st, n_pers, n_spmv, label):
    """which reduced solver ran.  The scope CCM_K_BA_PCG_PERSIST covers ba_solve_cholreg, ba_solve_dense2 AND ba_pcg_persist, so the count alone does not
    tell: a handle built for the register Cholesky has no persistent grid (pers_grid == 0, ba_build.hip), the two-cluster solve needs one and at most 32
    cameras, and both exact solvers report ONE iteration per trial (pcg_flag[1] = 1) where a PCG at 1e-8 takes many."""
    t = st.lm_trials
    if solver == "cholreg":
        ok = n_pers == t and n_spmv == 0 and sz["pers_grid"] == 0 and 16 < sz["Cp"] <= 50 and st.pcg_iters == t
    elif solver == "dense2":
        ok = n_pers == t and n_spmv == 0 and sz["pers_grid"] > 0 and 16 < sz["Cp"] <= 32 and st.pcg_iters == t
    elif solver == "pcg_small":
        ok = n_pers == 0 and n_spmv == t and sz["Cp"] <= 16 and st.pcg_iters > t
    elif solver == "pcg_persist":
        ok = n_pers == t and n_spmv == 0 and sz["pers_grid"] > 0 and sz["Cp"] > 50 and st.pcg_iters > t
    else:   # multi-kernel PCG
        ok = n_pers == 0 and n_spmv > t and sz["pers_grid"] == 0 and sz["Cp"] > 50 and st.pcg_iters > t
    assert ok, (label, solver, dict(n_pers=n_pers, n_spmv=n_spmv, pers_grid=sz["pers_grid"], Cp=sz["Cp"], pcg_iters=st.pcg_iters, trials=t))


def _one_trial(ctx, prob, scale, label, solver):
    sys0 = ref.reduced_system(prob, 1.0)
    lam = float(scale * sys0["max_diag"])
    sys = ref.reduced_system(prob, lam)
    stp = ref.lm_step(prob, sys, lam)
    lam_next, rho = ref.next_lambda(lam, sys["lin"]["chi2"], stp["chi2"], stp["scale"])
    assert rho > 0
    # the oracle's distance from the reference: the yardstick
    ocam, opts, ochi2, odpos, ost = oracle.ba_optimize(prob, 1, linear_solver=1, lambda_init=lam)
    assert ost.lm_trials == 1
    d_or, _ = _distances(ocam, opts, ochi2, odpos, ost.chi2_final, ost.lambda_hist[0], stp, lam_next)
    h = optimizer.BAHandle(ctx, prob)
    try:
        sz = h.debug_sizes()
        st, n_pers, n_spmv = _run(ctx, h, 1, lam)
        cam, pts, chi2, dpos = h.download()
        _, lam_hist, trials = h.history()
    finally:
        h.close()
    assert st.lm_trials == 1 and st.iters_done == 1 and trials[0] == 1, (label, st.lm_trials)
    _assert_solver(solver, sz, st, n_pers, n_spmv, label)
    assert sz["n_chunk"] > 0, (label, sz)                                    # ba_linearize_pts_e / ba_backsub_chi2_e
    n_act = sys["lin"]["edges"].size
    chi0 = sys["lin"]["chi2"]
    assert abs(LD(st.chi2_initial) - chi0) <= (n_act + ref.C_DEVICE) * ref.U53 * chi0, (label, st.chi2_initial, float(chi0))
    d_dev, dpos_ok = _distances(cam, pts, chi2, dpos, st.chi2_final, lam_hist[0], stp, lam_next)
    assert dpos_ok, label
    tol = _allowed(d_or)
    print(f"{label}: Cp {sz['Cp']} lambda {lam:.3g}")
    for k in d_dev:
        print(f"    {k:10s} device {d_dev[k]:.3e}  oracle {d_or[k]:.3e}  allowed {tol[k]:.3e}")
    for k in d_dev:
        assert d_dev[k] <= tol[k], (label, k, d_dev[k], d_or[k])
    assert st.lambda_final == lam_hist[0]
    return sz


@pytest.mark.parametrize("kfs", [19, 34, 51])
def test_one_trial_register_cholesky(ctx, kfs):
    """18, 33, 50 free cameras: ba_solve_cholreg"""
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=kfs, n_points=60 * kfs, seed=100 + kfs)
    sz = _one_trial(ctx, prob, 1e-3, f"cholreg {kfs - 1}", "cholreg")
    assert sz["Cp"] == kfs - 1


@pytest.mark.parametrize("kfs", [21, 33])
def test_one_trial_two_cluster_solve(ctx, kfs, monkeypatch):
    """20 and 32 free cameras with CCM_BA_CHOLREG=0 (read at create): ba_solve_dense2"""
    monkeypatch.setenv("CCM_BA_CHOLREG", "0")
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=kfs, n_points=60 * kfs, seed=200 + kfs)
    sz = _one_trial(ctx, prob, 1e-3, f"dense2 {kfs - 1}", "dense2")
    assert sz["Cp"] == kfs - 1


def test_first_lambda_follows_g2os_rule(ctx):
    """lambda_init = 0: the first lambda is 1e-5 x the largest diagonal entry of Hpp and Hll (ba_maxdiag).  The first trial is accepted on this map
    (the oracle's is too), so the lambda after the iteration is that value times the Levenberg factor of the reference step."""
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=26, n_points=1500, seed=300)
    lam0 = LD(1e-5) * ref.reduced_system(prob, 1.0)["max_diag"]
    s1 = ref.reduced_system(prob, float(lam0))
    stp = ref.lm_step(prob, s1, float(lam0))
    lam_next, rho = ref.next_lambda(lam0, s1["lin"]["chi2"], stp["chi2"], stp["scale"])
    assert rho > 0
    ost = oracle.ba_optimize(prob, 1, linear_solver=1)[4]
    assert ost.lm_trials == 1
    d_or = float(abs(LD(ost.lambda_hist[0]) - lam_next) / lam_next)
    h = optimizer.BAHandle(ctx, prob)
    try:
        st = h.run(1)
        _, lam_hist, trials = h.history()
    finally:
        h.close()
    assert st.lm_trials == 1 and trials[0] == 1
    d_dev = float(abs(LD(lam_hist[0]) - lam_next) / lam_next)
    print(f"first lambda: device {lam_hist[0]!r} reference {float(lam_next)!r} distance {d_dev:.3e} oracle {d_or:.3e}")
    assert d_dev <= MARGIN * max(d_or, LAM_NEXT_FLOOR), (lam_hist[0], float(lam_next), d_dev, d_or)


def test_two_iterations_use_the_fused_dinv(ctx):
    """run(2), both iterations accepted at the first trial, against two reference steps in a row: from the second iteration on ba_linearize_pts_e forms
    D^-1 and D^-1 b_l itself for the lambda it is handed, a path no hook reaches"""
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=31, n_points=1800, seed=400)
    lam = float(1e-3 * ref.reduced_system(prob, 1.0)["max_diag"])
    s1 = ref.reduced_system(prob, lam)
    t1 = ref.lm_step(prob, s1, lam)
    lam2, rho1 = ref.next_lambda(lam, s1["lin"]["chi2"], t1["chi2"], t1["scale"])
    # (the second step starts from the reference's own first step rounded to f64, which is how the device and the oracle hold a state)
    s2 = ref.reduced_system(prob, float(lam2), cam_qt=t1["cam"], pt_xyz=t1["pts"])
    t2 = ref.lm_step(prob, s2, float(lam2), cam_qt=t1["cam"], pt_xyz=t1["pts"])
    lam3, rho2 = ref.next_lambda(lam2, t1["chi2"], t2["chi2"], t2["scale"])
    assert rho1 > 0 and rho2 > 0
    ocam, opts, ochi2, odpos, ost = oracle.ba_optimize(prob, 2, linear_solver=1, lambda_init=lam)
    assert ost.lm_trials == 2 and ost.iters_done == 2
    d_or, _ = _distances(ocam, opts, ochi2, odpos, ost.chi2_final, ost.lambda_hist[1], t2, lam3)
    h = optimizer.BAHandle(ctx, prob)
    try:
        sz = h.debug_sizes()
        assert sz["n_chunk"] > 0
        st, n_pers, n_spmv = _run(ctx, h, 2, lam)
        cam, pts, chi2, dpos = h.download()
        _, lam_hist, trials = h.history()
    finally:
        h.close()
    assert st.lm_trials == 2 and st.iters_done == 2
    _assert_solver("cholreg", sz, st, n_pers, n_spmv, "two iterations")
    d_dev, dpos_ok = _distances(cam, pts, chi2, dpos, st.chi2_final, lam_hist[1], t2, lam3)
    assert dpos_ok
    tol = _allowed(d_or)
    for k in d_dev:
        print(f"two iterations: {k:10s} device {d_dev[k]:.3e}  oracle {d_or[k]:.3e}  allowed {tol[k]:.3e}")
    for k in d_dev:
        assert d_dev[k] <= tol[k], (k, d_dev[k], d_or[k])


# ---- PCG-solved maps ------------------------------------------------------------------------------------------------------------------
REL_TOL = 1e-8


def _camera_steps(prob, sys, cam_new):
    """dx with exp(dx) T_old = T_new for every free camera of the reference, by the long-double log map"""
    old = ref._ld(prob["cam_qt"]); new = ref._ld(cam_new)
    out = np.zeros((sys["cams"].size, 6), LD)
    for k, c in enumerate(sys["cams"]):
        qo = old[c, :4] / np.sqrt((old[c, :4] ** 2).sum())
        q = ref.quat_mul(new[c, :4], np.array([-qo[0], -qo[1], -qo[2], qo[3]], LD))
        R = ref.rot_from_quat(q[None])[0]
        out[k] = ref.se3_log(q, new[c, 4:] - R @ old[c, 4:])
    return out


def _pcg_trial(ctx, prob, scale, label, solver, expect_chunks=True):
    lam = float(scale * ref.reduced_system(prob, 1.0)["max_diag"])
    sys = ref.reduced_system(prob, lam)
    h = optimizer.BAHandle(ctx, prob)
    try:
        sz = h.debug_sizes()
        st, n_pers, n_spmv = _run(ctx, h, 1, lam, pcg_rel_tol=REL_TOL)
        cam, pts, chi2, dpos = h.download()
    finally:
        h.close()
    assert st.lm_trials == 1 and st.iters_done == 1, (label, st.lm_trials)
    _assert_solver(solver, sz, st, n_pers, n_spmv, label)
    assert (sz["n_chunk"] > 0) == expect_chunks, (label, sz)                # ba_linearize_pts_e + ba_backsub_chi2_e, or the per-landmark kernels
    n_act = sys["lin"]["edges"].size
    chi0 = sys["lin"]["chi2"]
    assert abs(LD(st.chi2_initial) - chi0) <= (n_act + ref.C_DEVICE) * ref.U53 * chi0, (label, st.chi2_initial, float(chi0))
    # the camera step as a residual of the reference's system
    dx = _camera_steps(prob, sys, cam)
    A = ref.dense(sys, lam)
    b = sys["b"].ravel()
    res = float(np.sqrt(((A @ dx.ravel() - b) ** 2).sum()) / np.sqrt((b * b).sum()))
    print(f"{label}: Cp {sz['Cp']} lambda {lam:.3g} pcg iterations {st.pcg_iters} relative residual {res:.3e} (allowed {2 * REL_TOL:.1e})")
    assert res <= 2 * REL_TOL, (label, res)
    # the landmark step for THAT camera step: (n + c) 2^-53 |.|_acc, plus the two roundings of X + dx to f64 and of the difference taken here
    dx_l, dx_l_abs, n_l = ref.landmark_step(sys, dx)
    X_old = ref._ld(prob["pt_xyz"])[sys["pts"]]; X_new = ref._ld(pts)[sys["pts"]]
    bound = (n_l.astype(LD)[:, None] + ref.C_DEVICE) * ref.U53 * dx_l_abs + 2 * ref.U53 * np.abs(X_new)
    err = np.abs((X_new - X_old) - dx_l)
    w = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"    landmark step: largest used share of the bound {float((err / bound)[w]):.3f}")
    assert np.all(err <= bound), (label, int(sys["pts"][w[0]]), int(w[1]), float(err[w]), float(bound[w]), float(dx_l[w]))
    # chi2 and the per-edge chi2 of the trial, against the reference AT the downloaded state
    lin = ref.linearize(prob, cam, pts)
    assert abs(LD(st.chi2_final) - lin["chi2"]) <= (n_act + ref.C_DEVICE) * ref.U53 * lin["chi2"], (label, st.chi2_final, float(lin["chi2"]))
    # per edge: |e| carries the rounding of obs - proj, about 16 operations on numbers of the size of the pixel coordinates
    Kc = ref._ld(prob["cam_K"])[lin["e_cam"]]
    mag = np.abs(ref._ld(prob["e_obs"])[lin["edges"]]) + np.abs(lin["e"]) + np.abs(Kc[:, 2:4])
    e_bound = 2 * lin["info"] * (np.abs(lin["e"]) * 16 * ref.U53 * mag).sum(1) + 4 * ref.U53 * lin["e2"]
    e_err = np.abs(chi2[lin["edges"]].astype(LD) - lin["e2"])
    assert np.all(e_err <= e_bound), (label, float((e_err / e_bound).max()))
    assert np.array_equal(dpos[lin["edges"]] != 0, lin["Xc"][:, 2] > 0)
    assert LD(st.chi2_final) < chi0
    return sz


def test_one_trial_single_workgroup_pcg(ctx):
    """11 free cameras: ba_pcg_small"""
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=12, n_points=700, seed=500)
    sz = _pcg_trial(ctx, prob, 1e-3, "pcg_small 11", "pcg_small")
    assert sz["Cp"] == 11


def test_one_trial_persistent_pcg(ctx):
    """179 free cameras: ba_pcg_persist"""
    prob = synth.make_ba_problem(n_agents=3, kfs_per_agent=60, n_points=6000, seed=11)
    sz = _pcg_trial(ctx, prob, 1e-3, "pcg_persist 179", "pcg_persist")
    assert sz["Cp"] == 179


def test_one_trial_multi_kernel_pcg(ctx, monkeypatch):
    """the same map with CCM_BA_NO_PERSIST=1 (read at create): the multi-kernel PCG"""
    monkeypatch.setenv("CCM_BA_NO_PERSIST", "1")
    prob = synth.make_ba_problem(n_agents=3, kfs_per_agent=60, n_points=6000, seed=11)
    sz = _pcg_trial(ctx, prob, 1e-3, "multi-kernel 179", "multi_kernel")
    assert sz["Cp"] == 179


def test_one_trial_with_a_257_observation_landmark(ctx):
    """a landmark above the chunked kernels' limit inside a real trial: ba_linearize_pts and ba_backsub_chi2 (n_chunk == 0); 258 free cameras, so the
    reduced solve is the persistent PCG and the step is judged like the other PCG cases"""
    prob = _one_long_track(257)
    sz = _pcg_trial(ctx, prob, 1e-3, "257-observation landmark", "pcg_persist", expect_chunks=False)
    assert sz["n_chunk"] == 0 and sz["Cp"] == 258
