"""The persistent PCG's Chronopoulos-Gear recurrence (ba_pcg_persist, ba.hip) restated in numpy next to the textbook
two-reduction PCG it replaced, on synthetic reduced camera systems shaped like the bundle adjustment's: 6x6 blocks,
covisibility-banded, preconditioned by 96-unknown cluster-Jacobi (16 cameras per cluster) plus the additive hat coarse
space of the persistent kernel.  Both loops must take the same number of iterations (+-1) and reach the same solution;
an indefinite system must take the p^T A p <= 0 failure exit."""
import numpy as np
import pytest

CLU = 96   # unknowns per preconditioner cluster (kCluN)


def _system(n_cam, band, seed, indefinite=False):
    """A reduced camera system like the Schur complement of BA: a sum of PSD edge terms [G, -G]^T [G, -G] between
    covisible cameras (nearly singular along the smooth, map-wide motions that the coarse space targets) plus a small
    per-camera term."""
    rng = np.random.default_rng(seed)
    n = 6 * n_cam
    S = np.zeros((n, n))
    for i in range(n_cam):
        for j in range(i + 1, min(n_cam, i + band + 1)):
            if j == i + 1 or rng.random() < 0.5:
                G = rng.standard_normal((6, 6)) / (j - i)
                H = G.T @ G
                bi, bj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
                S[bi, bi] += H; S[bj, bj] += H; S[bi, bj] -= H; S[bj, bi] -= H
        G = rng.standard_normal((6, 6)) * 0.05
        S[6 * i:6 * i + 6, 6 * i:6 * i + 6] += G.T @ G
    if indefinite:
        S[:6, :6] -= np.eye(6) * (np.abs(S).sum() + 1.0)
    b = rng.standard_normal(n)
    return S, b


def _precond(A, n_cam, agg, coarse):
    """M^-1 as the persistent kernel applies it: cluster-Jacobi blocks plus P Ac^-1 P^T on the hat coarse space."""
    n = A.shape[0]
    blocks = [(s, min(n, s + CLU)) for s in range(0, n, CLU)]
    W = [np.linalg.inv(A[s:e, s:e]) for s, e in blocks]
    P = None
    if coarse:
        na = (n_cam + agg - 1) // agg
        P = np.zeros((n, 6 * (na + 1)))
        for k in range(n_cam):
            t = ((k % agg) + 0.5) / agg
            nd = k // agg
            P[6 * k:6 * k + 6, 6 * nd:6 * nd + 6] = (1.0 - t) * np.eye(6)
            P[6 * k:6 * k + 6, 6 * nd + 6:6 * nd + 12] = t * np.eye(6)
        Ainv = np.linalg.inv(P.T @ A @ P)

    def apply(r):
        z = np.concatenate([Wb @ r[s:e] for Wb, (s, e) in zip(W, blocks)])
        if P is not None:
            z = z + P @ (Ainv @ (P.T @ r))
        return z
    return apply


def pcg_two_exchanges(A, b, M, tol, max_it):
    """The loop the persistent kernel ran before: reductions for p.q and for r.z in every iteration."""
    x = np.zeros_like(b); r = b.copy(); z = M(r); rz = r @ z; rz0 = rz; p = np.zeros_like(b)
    k = 0
    while k < max_it:
        if rz <= tol * tol * rz0 or not rz > 0:
            break
        beta = 0.0 if k == 0 else rz / rz_prev
        p = z + beta * p
        q = A @ p
        pq = p @ q
        if not pq > 0:
            return x, k, True
        alpha = rz / pq
        x += alpha * p; r -= alpha * q
        z = M(r)
        rz_prev = rz; rz = r @ z
        k += 1
    return x, k, False


def pcg_one_exchange(A, b, M, tol, max_it):
    """Chronopoulos-Gear: one reduction of (gamma, delta) = ((r, u), (w, u)) per iteration, s = A p by recurrence."""
    x = np.zeros_like(b); r = b.copy(); p = np.zeros_like(b); s = np.zeros_like(b)
    u = M(r); w = A @ u
    gam, dl = r @ u, w @ u
    gam0 = gam
    k = 0
    while k < max_it:
        if gam <= tol * tol * gam0 or not gam > 0:
            break
        beta = 0.0 if k == 0 else gam / gam_prev
        pap = dl if k == 0 else dl - beta * gam / alpha_prev
        if not pap > 0:
            return x, k, True
        alpha = gam / pap
        p = u + beta * p; s = w + beta * s
        x += alpha * p; r -= alpha * s
        u = M(r); w = A @ u
        gam_prev, alpha_prev = gam, alpha
        gam, dl = r @ u, w @ u
        k += 1
    return x, k, False


@pytest.mark.parametrize("coarse", [False, True])
@pytest.mark.parametrize("lam", [1e-3, 1e-1, 1e1, 1e3])
@pytest.mark.parametrize("seed", [0, 1])
def test_one_exchange_recurrence_matches_two_exchange_pcg(coarse, lam, seed):
    n_cam = 80
    S, b = _system(n_cam, band=6, seed=seed)
    A = S + lam * np.eye(S.shape[0])
    M = _precond(A, n_cam, agg=16, coarse=coarse)
    tol = 1e-8
    x2, k2, f2 = pcg_two_exchanges(A, b, M, tol, 500)
    x1, k1, f1 = pcg_one_exchange(A, b, M, tol, 500)
    assert not f1 and not f2
    assert abs(k1 - k2) <= 1, (k1, k2)
    xe = np.linalg.solve(A, b)
    # both at the tolerance of the preconditioned residual: the solutions agree to well within it
    scale = np.linalg.norm(xe)
    assert np.linalg.norm(x1 - x2) <= 1e-6 * scale
    assert np.linalg.norm(A @ x1 - b) <= 1e-6 * np.linalg.norm(b)


def test_indefinite_system_takes_the_failure_exit():
    n_cam = 32
    S, b = _system(n_cam, band=4, seed=3, indefinite=True)
    A = S + 1e-3 * np.eye(S.shape[0])
    # an SPD preconditioner (the cluster blocks of the indefinite matrix itself are not): both loops must stop on
    # p^T A p <= 0 rather than return a solution
    c = np.abs(A).sum()
    M = lambda r: r / c
    _, _, f2 = pcg_two_exchanges(A, b, M, 1e-8, 500)
    _, _, f1 = pcg_one_exchange(A, b, M, 1e-8, 500)
    assert f2 and f1
