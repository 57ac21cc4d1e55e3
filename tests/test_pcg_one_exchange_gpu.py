"""The persistent PCG (ba_pcg_persist: Chronopoulos-Gear CG, one grid-wide exchange per iteration, self-validating halo
exchange of u) on the device, through the test hook ccm_ba_debug_pcg_solve: one solve of (S + lambda I) x = b at the
current state.  Checked against the reduced system the handle itself built (ccm_ba_debug_partial_reduced) and a numpy
PCG with the same preconditioner (16-camera cluster-Jacobi plus the hat coarse level of ccm_ba_debug_coarse).  A launch
that gave up waiting for its peers (pcg_flag[3]) fails the test here instead of being repeated on the multi-kernel path,
and the LM runs below assert that no trial fell back."""
import ctypes as C

import numpy as np
import pytest

from ccm_slam_amd import optimizer, synth
from ccm_slam_amd._lib import K, hooks
from tests.test_ba_structure_gpu import dev_array

CLU = 16   # cameras per preconditioner cluster (kClu)
AGG = 16   # cameras per coarse interval on the persistent solver's path


def _pers_solve(h, lam, coarse, tol=1e-8, max_it=1000):
    n = 6 * h.counts()["free_cams"]
    x = np.zeros(n)
    fl = np.zeros(4, np.int32)
    rc = hooks().ccm_ba_debug_pcg_solve(h._h, C.c_double(lam), int(coarse), C.c_double(tol), int(max_it), x.ctypes.data_as(C.c_void_p),
                                        C.c_size_t(n), fl.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return x, fl


def _reduced(h, lam):
    """S blocks (without lambda), their block rows / columns, and b of the handle's reduced system."""
    red = h.partial_reduced(lam)
    n = 6 * h.counts()["free_cams"]
    nb = (red.size - n) // 36
    B = red[:36 * nb].reshape(nb, 6, 6)
    bi = dev_array(h, "blk_i", np.int32)[:nb].astype(np.int64)
    bj = dev_array(h, "blk_j", np.int32)[:nb].astype(np.int64)
    return B, bi, bj, red[36 * nb:36 * nb + n].copy()


def _matvec(B, bi, bj, lam, x):
    X = x.reshape(-1, 6)
    Y = lam * X
    np.add.at(Y, bi, np.einsum("bij,bj->bi", B, X[bj]))
    off = bi != bj
    np.add.at(Y, bj[off], np.einsum("bji,bj->bi", B[off], X[bi[off]]))
    return Y.ravel()


def _precond(h, B, bi, bj, lam, coarse):
    Cp = h.counts()["free_cams"]
    ncl = (Cp + CLU - 1) // CLU
    W = []
    for c in range(ncl):
        lo, hi = c * CLU, min(Cp, (c + 1) * CLU)
        A = lam * np.eye(6 * (hi - lo))
        for k in np.flatnonzero((bi // CLU == c) & (bj // CLU == c)):
            i, j = bi[k] - lo, bj[k] - lo
            A[6 * i:6 * i + 6, 6 * j:6 * j + 6] += B[k]
            if i != j:
                A[6 * j:6 * j + 6, 6 * i:6 * i + 6] += B[k].T
        W.append(np.linalg.inv(A))
    Pd = Ai = None
    if coarse:
        na, _, Ai, P = h.coarse_level(lam)
        Pd = np.zeros((6 * Cp, 6 * (na + 1)))
        for i in range(Cp):
            a, w1 = i // AGG, ((i % AGG) + 0.5) / AGG
            Pk = P[i].reshape(6, 6)
            Pd[6 * i:6 * i + 6, 6 * a:6 * a + 6] = (1 - w1) * Pk
            Pd[6 * i:6 * i + 6, 6 * (a + 1):6 * (a + 1) + 6] = w1 * Pk

    def apply(r):
        z = np.concatenate([W[c] @ r[6 * c * CLU:6 * c * CLU + W[c].shape[0]] for c in range(ncl)])
        if Pd is not None:
            z = z + Pd @ (Ai @ (Pd.T @ r))
        return z
    return apply


def _numpy_pcg(Av, b, M, tol, max_it=1000):
    x = np.zeros_like(b); r = b.copy(); z = M(r); rz = r @ z; rz0 = rz; p = np.zeros_like(b)
    k = 0
    while k < max_it and rz > tol * tol * rz0:
        beta = 0.0 if k == 0 else rz / rz_prev
        p = z + beta * p
        q = Av(p)
        alpha = rz / (p @ q)
        x += alpha * p; r -= alpha * q
        z = M(r)
        rz_prev, rz = rz, r @ z
        k += 1
    return x, k


def _problem(name):
    if name == "map179":   # 3 agents x 60 keyframes: 179 free cameras, 6 coarse intervals
        return synth.make_ba_problem(n_agents=3, kfs_per_agent=60, n_points=6000, seed=11)
    return synth.make_ba_config(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["map179", "gba_c3"])
def test_persistent_solve_reaches_the_tolerance(ctx, name):
    """Coarse level on and off, lambda from 1e-7 to 1e-1 of the largest diagonal entry (the LM loop starts at 1e-5 and moves both ways): the solve ends
    clean (no give-up, no numeric failure), its true residual is within 10x that of a numpy PCG with the same preconditioner, and it takes the
    same number of iterations within 2 (the device keeps the coarse inverse's rows in f32 and sums in another order)."""
    prob = _problem(name)
    h = optimizer.BAHandle(ctx, prob)
    try:
        B0, bi, bj, _ = _reduced(h, 1.0)
        dmax = max(np.diagonal(B0[k]).max() for k in np.flatnonzero(bi == bj))
        assert h.coarse_level(1.0)[0] > 0
        for scale in (1e-7, 1e-5, 1e-3, 1e-1):
            lam = scale * dmax
            B, bi, bj, b = _reduced(h, lam)
            Av = lambda v: _matvec(B, bi, bj, lam, v)
            for coarse in (True, False):
                x, fl = _pers_solve(h, lam, coarse)
                assert fl[3] == 0 and fl[2] == 0 and fl[1] > 0, (scale, coarse, fl)
                xr, kr = _numpy_pcg(Av, b, _precond(h, B, bi, bj, lam, coarse), 1e-8)
                res, res_ref = np.linalg.norm(Av(x) - b), np.linalg.norm(Av(xr) - b)
                assert res <= 10 * res_ref + 1e-12 * np.linalg.norm(b), (scale, coarse, res, res_ref)
                assert abs(int(fl[1]) - kr) <= 2, (scale, coarse, int(fl[1]), kr)
    finally:
        h.close()


def _lm_run(ctx, prob, iters):
    h = optimizer.BAHandle(ctx, prob)
    ctx.prof_enable(-1); ctx.prof_reset()
    st = h.run(iters)
    n_pers, _ = ctx.prof_read(K["BA_PCG_PERSIST"])
    n_spmv, _ = ctx.prof_read(K["BA_PCG_SPMV"])
    ctx.prof_enable(-2)
    cam, _, _, _ = h.download()
    h.close()
    return st, cam, n_pers, n_spmv


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gba_c3", "lba62"])
def test_persistent_and_multi_kernel_solvers_take_the_same_lm_path(ctx, name, monkeypatch):
    """The persistent solver against the multi-kernel one (CCM_BA_NO_PERSIST, read at create time) on gba_c3 and on a 62-camera local BA: same LM
    iterations and trials, poses within 5e-9 (the bar of test_formulations_of_the_large_map_path_agree), and the persistent run never fell back."""
    if name == "lba62":
        prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=70, n_points=4000, n_fixed=8, fixed_mode="tail", seed=2062)
    else:
        prob = synth.make_ba_config(name)
    st_p, cam_p, n_pers, n_spmv = _lm_run(ctx, prob, 10)
    assert n_pers > 0 and n_spmv == 0, (n_pers, n_spmv)
    monkeypatch.setenv("CCM_BA_NO_PERSIST", "1")
    st_m, cam_m, n_pers_m, n_spmv_m = _lm_run(ctx, prob, 10)
    assert n_pers_m == 0 and n_spmv_m > 0
    assert (st_p.iters_done, st_p.lm_trials) == (st_m.iters_done, st_m.lm_trials)
    assert np.abs(cam_p - cam_m).max() < 5e-9, np.abs(cam_p - cam_m).max()
