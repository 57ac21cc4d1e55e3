"""GPU box: the dense inverse / dense solve / tile-sparse solve test hooks on a fixed list of small SPD matrices, with whatever CCM_CHOL_* switches the
environment carries (they are read once per process, hence a process per variant); every result goes into ONE .npz.  tests/test_dense_chain_gpu.py runs the
same list in its own process and in a child with CCM_CHOL_CHAIN=split and compares the arrays bit for bit.
usage: dense_chain_run.py <out.npz>"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SIZES = (64, 65, 130, 200, 756)   # one tile / first panel, update and L^-1 step with padding rows / first off-diagonal pair, two-term L^-1 sum / four tile rows / flagship
PIVOTS = ((70, 40), (130, 129))   # (n, row of the non-positive pivot): first tile, third tile


def spd(n):
    rng = np.random.default_rng(n)
    M = rng.normal(size=(n, n))
    return M @ M.T + n * np.eye(n), rng.normal(size=n)


def int_spd(n, band):
    """integer-valued, banded, diagonally dominant: every entry is exact in f64 whatever the host's summation order, so results recorded on one machine
    (tests/golden/dense_chain_parent.npz, from the commit before the fused chain) can be compared bit for bit on another"""
    i, j = np.arange(n, dtype=np.int64)[:, None], np.arange(n, dtype=np.int64)[None, :]
    M = ((i * 131 + j * 71 + (i * j) % 97 * 17) % 17 - 8) * (np.abs(i - j) <= band)
    A = M + M.T
    A += np.diag(np.abs(A).sum(axis=1) + 1)
    return A.astype(np.float64), ((np.arange(n) * 37) % 11 - 5).astype(np.float64)


def tile_case():
    """banded, 5 tile rows: the tile-sparse solver's diagonal body with gathers of one and two terms"""
    return int_spd(300, 90)


def gold_inverse_case():
    """dense, 3 tile rows with padding: the whole inverse chain"""
    return int_spd(130, 130)


def run_cases(ctx):
    from ccm_slam_amd import optimizer
    out = {}
    for n in SIZES:
        A, b = spd(n)
        out[f"ainv_{n}"], out[f"ainv_info_{n}"] = optimizer.debug_dense_inverse(ctx, A)
        out[f"x_{n}"], out[f"x_info_{n}"] = optimizer.debug_dense_solve(ctx, A, b)
    for n, row in PIVOTS:
        A = np.eye(n); A[row, row] = -1.0
        _, out[f"pivot_inv_{n}"] = optimizer.debug_dense_inverse(ctx, A)
        _, out[f"pivot_solve_{n}"] = optimizer.debug_dense_solve(ctx, A, np.ones(n))
    A, b = tile_case()
    out["tile_x"], out["tile_info"], _, _ = optimizer.debug_tile_solve(ctx, A, b)
    A, _ = gold_inverse_case()
    out["gold_ainv"], out["gold_ainv_info"] = optimizer.debug_dense_inverse(ctx, A)
    return {k: np.asarray(v) for k, v in out.items()}


if __name__ == "__main__":
    from ccm_slam_amd._lib import Context
    ctx = Context(0)
    np.savez(sys.argv[1], **run_cases(ctx))
    ctx.close()
