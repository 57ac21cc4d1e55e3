"""Reference of the dense / tile-sparse Cholesky family of ccm_slam_amd/csrc/dense_chol.hip, written from the textbook formulas
(Golub & Van Loan, Alg. 4.2.1; Higham, Accuracy and Stability, ch. 7 and 10), not from the kernels: unblocked, one column at a
time, plain NumPy, parameterised by dtype (float64: the yardstick of what f64 gives; numpy.longdouble, 64-bit mantissa on x86
(`HAVE_EXTENDED`): the truth the device is measured against).  No GPU, no library call.

    factor(A, dtype)            L, first failing column (-1: none), smallest pivot
    solve(A, b, dtype)          x, first failing column
    inverse(A, dtype)           A^-1 = L^-T L^-1, first failing column
    first_failing_pivot(A)      LAPACK's report: the smallest column whose pivot is not > 0 (and finite)
    tile_symbolic(nz)           filled tile pattern, elimination level of every tile column, `levels` and `tiles` of the plan
    eta / rho / cond_inf        the error measures, in long double
    cases()                     THE case list: tests/test_chol_edges_gpu.py and scripts/chol_edges_run.py both take it from here
"""
from __future__ import annotations

import functools

import numpy as np

LD = np.longdouble
HAVE_EXTENDED = np.finfo(LD).nmant >= 63
U53 = 2.0 ** -53
NB = 64                  # tile size of the device's forms
MAX_ROWS = 518


# ---------------------------------------------------------------------------------------------------------------- numerics
def _pivot_ok(d) -> bool:
    return bool(d > 0) and bool(np.isfinite(d))


def factor(A, dtype=LD):
    """A = L L^T, column by column.  Returns (L, bad, dmin): bad = the smallest column whose pivot (the diagonal entry after the
    earlier columns were eliminated) is not positive and finite, -1 if there is none; the factorisation stops there (LAPACK's
    potrf: the leading minor of that order is not positive definite).  dmin = smallest accepted pivot."""
    with np.errstate(all="ignore"):
        A = np.asarray(A, np.float64).astype(dtype)
        n = A.shape[0]
        L = np.zeros((n, n), dtype)
        dmin = dtype(np.inf)
        for j in range(n):
            row = L[j, :j]
            d = A[j, j] - row @ row
            if not _pivot_ok(d):
                return L, j, dmin
            dmin = min(dmin, d)
            ljj = np.sqrt(d)
            L[j, j] = ljj
            if j + 1 < n:
                L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ row) / ljj
        return L, -1, dmin


def first_failing_pivot(A, dtype=LD) -> int:
    return factor(A, dtype)[1]


def forward(L, b):
    """y with L y = b (b: vector or matrix of columns)"""
    y = np.array(b, dtype=L.dtype)
    for i in range(L.shape[0]):
        y[i] = (y[i] - L[i, :i] @ y[:i]) / L[i, i]
    return y


def backward(L, y):
    """x with L^T x = y"""
    x = np.array(y, dtype=L.dtype)
    for i in range(L.shape[0] - 1, -1, -1):
        x[i] = (x[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


def solve(A, b, dtype=LD):
    L, bad, _ = factor(A, dtype)
    if bad >= 0:
        return None, bad
    return backward(L, forward(L, np.asarray(b, np.float64).astype(dtype))), -1


def inverse(A, dtype=LD):
    L, bad, _ = factor(A, dtype)
    if bad >= 0:
        return None, bad
    X = forward(L, np.eye(L.shape[0], dtype=dtype))      # L^-1
    return X.T @ X, -1


def _ld(a):
    return np.asarray(a, np.float64).astype(LD)


def norm_inf(M) -> LD:
    M = np.asarray(M)
    return np.abs(M).sum(axis=1).max() if M.ndim == 2 else np.abs(M).max()


def eta(A, x, b) -> float:
    """normwise backward error of a solve (Rigal & Gaches): |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), in long double"""
    A, x, b = _ld(A), _ld(x), _ld(b)
    return float(norm_inf(b - A @ x) / (norm_inf(A) * norm_inf(x) + norm_inf(b)))


def rho(A, X) -> float:
    """right residual of an inverse: |A X - I|_inf / (|A|_inf |X|_inf), in long double"""
    A, X = _ld(A), _ld(X)
    return float(norm_inf(A @ X - np.eye(A.shape[0], dtype=LD)) / (norm_inf(A) * norm_inf(X)))


def cond_inf(A, Ainv_ld) -> float:
    return float(norm_inf(_ld(A)) * norm_inf(Ainv_ld))


# ---------------------------------------------------------------------------------------------------------- symbolic, by tiles
def tile_pattern(A, nb: int = NB):
    """T x T lower-triangular boolean pattern of the nb x nb tiles of A that hold a non-zero (NaN counts), diagonal always set"""
    A = np.asarray(A)
    n = A.shape[0]
    T = -(-n // nb)
    P = np.zeros((T * nb, T * nb), bool)
    P[:n, :n] = A != 0
    nz = P.reshape(T, nb, T, nb).any(axis=(1, 3))
    return np.tril(nz | nz.T | np.eye(T, dtype=bool))


def tile_symbolic(nz):
    """Symbolic Cholesky of a tile pattern (lower triangle, T x T boolean): the structure of column j of L is the union of the
    pattern of column j of A and of the structures of the columns k < j that have a tile in row j, without the rows <= j.
    Returns dict(fill: pattern of L, level[j]: 0 if row j of L is empty, else 1 + the deepest column it has a tile in,
    levels = number of levels, tiles = non-zero tiles of L with the diagonal)."""
    nz = np.asarray(nz, bool)
    T = nz.shape[0]
    struct = [set(int(i) for i in np.nonzero(nz[:, j])[0] if i > j) for j in range(T)]
    for j in range(T):
        for k in range(j):
            if j in struct[k]:
                struct[j] |= {i for i in struct[k] if i > j}
    level = [0] * T
    for j in range(T):
        left = [k for k in range(j) if j in struct[k]]
        level[j] = 1 + max(level[k] for k in left) if left else 0
    fill = np.eye(T, dtype=bool)
    for j in range(T):
        for i in struct[j]:
            fill[i, j] = True
    return dict(fill=fill, level=level, levels=max(level) + 1, tiles=T + sum(len(s) for s in struct))


# ------------------------------------------------------------------------------------------------------------------ the cases
def _sym(A):
    return (A + A.T) * 0.5        # a + b == b + a in floating point: exactly symmetric


def _rhs(rng, n):
    return rng.normal(size=n)


def random_spd(n, seed):
    """M M^T + n I: condition number about 5"""
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(n, n))
    return _sym(M @ M.T + n * np.eye(n)), _rhs(rng, n)


def graded_spd(n, kappa, seed):
    """Q diag(kappa^(-i / (n - 1))) Q^T with a seeded orthogonal Q: spectrum graded from 1 down to 1 / kappa"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    d = np.float64(kappa) ** (-np.arange(n) / (n - 1.0))
    return _sym((Q * d) @ Q.T), _rhs(rng, n)


def chain_spd(F, lam, seed):
    """kron(L_F, I_7) + lam I: L_F the Laplacian of a path of F vertices hanging on one grounded end (2 on the diagonal, 1 at the free
    end, -1 beside it): the pose graph's own shape, 7 unknowns per keyframe, lambda_min ~ (pi / 2F)^2"""
    Lf = 2.0 * np.eye(F) - np.eye(F, k=1) - np.eye(F, k=-1)
    Lf[F - 1, F - 1] = 1.0
    A = np.kron(Lf, np.eye(7)) + lam * np.eye(7 * F)
    return _sym(A), _rhs(np.random.default_rng(seed), 7 * F)


def pattern_spd(P, n, seed):
    """values as tests/test_posegraph_gpu.py::_spd_with_pattern (M + M^T masked, then diagonally dominant) on the tile pattern P"""
    P = np.asarray(P, bool)
    P = P | P.T | np.eye(P.shape[0], dtype=bool)
    t = np.arange(n) // NB
    mask = P[t[:, None], t[None, :]].astype(np.float64)
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(n, n)) * mask
    A = M + M.T
    A += np.diag(np.abs(A).sum(axis=1) + 1.0)
    return A, _rhs(rng, n)


def _pat(T, pairs):
    P = np.zeros((T, T), bool)
    for i, j in pairs:
        P[i, j] = True
    return P


def bordered_pattern():
    """diagonal blocks of 1, 2 and 3 tiles (dense inside), bordered by two tile rows: T = 8; block {3, 4, 5} is three levels deep"""
    blocks = ((0,), (1, 2), (3, 4, 5))
    pairs = [(i, j) for blk in blocks for i in blk for j in blk]
    pairs += [(i, j) for i in (6, 7) for j in range(8)]
    return _pat(8, pairs)


def tile_patterns():
    """name -> (tile pattern, n)"""
    rng = np.random.default_rng(2024)
    rand = np.tril(rng.random((8, 8)) < 0.3, -1)
    return {
        "block_diagonal": (_pat(4, []), 256),                                                   # every column on level 0; ends on a tile edge
        "wrong_way_arrow": (_pat(6, [(i, 0) for i in range(6)]), 373),                          # dense first tile column: full fill
        "two_chains": (_pat(8, [(1, 0), (2, 1), (4, 3), (5, 4), (6, 5), (7, 6)]), 500),         # depths 3 and 5, independent
        "bordered_unequal": (bordered_pattern(), 482),
        "random": (rand, 450),
        "one_tile": (_pat(1, []), 64),
    }


SIZES = (1, 2, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128, 129, 192, 193, 257)
GRADED = [(n, k) for k in (1.0, 1e4, 1e8, 1e12) for n in (65, 129, 193)] + [(257, 1e12)]
CHAINS = [(F, lam) for F in (9, 10, 37, 74) for lam in (0.0, 1e-9)]


def _neg_diag(n, rows, seed):
    A, b = random_spd(n, seed)
    for r in rows:
        A[r, r] = -1.0
    return A, b


def _zero_pivot(n, r, seed):
    """row and column r emptied: the pivot is 0 - sum of (0 / l)^2 = exactly 0 in any arithmetic"""
    A, b = random_spd(n, seed)
    A[r, :] = 0.0
    A[:, r] = 0.0
    return A, b


def _minor(n, p, seed):
    """[[1, 2], [2, 1]] at rows (p, p + 1), decoupled from the rest: every diagonal entry is positive, the pivot of p + 1 is 1 - 4"""
    A, b = random_spd(n, seed)
    for r in (p, p + 1):
        A[r, :] = 0.0
        A[:, r] = 0.0
    A[p, p] = A[p + 1, p + 1] = 1.0
    A[p, p + 1] = A[p + 1, p] = 2.0
    return A, b


def _put(n, entries, seed):
    A, b = random_spd(n, seed)
    for i, j, v in entries:
        A[i, j] = A[j, i] = v
    return A, b


@functools.lru_cache(maxsize=1)
def cases():
    """The list.  Every case: dict(name, kind, A, b) with kind "ok" (must succeed in every form), "fail" (finite; info must be the
    reference's first failing column + 1 in every form) or "nonfinite".  Matrices are built from a seed, exactly symmetric and at
    most MAX_ROWS rows; callers must not write to them."""
    out = []

    def add(name, kind, Ab):
        A, b = Ab
        assert A.shape[0] <= MAX_ROWS and (np.array_equal(A, A.T) or kind == "nonfinite")
        A.setflags(write=False)
        b.setflags(write=False)
        out.append(dict(name=name, kind=kind, A=A, b=b))

    for n in SIZES:
        add(f"spd_{n}", "ok", random_spd(n, 1000 + n))
    for n, k in GRADED:
        add(f"graded_{n}_k{k:.0e}", "ok", graded_spd(n, k, 2000 + n))
    for F, lam in CHAINS:
        add(f"chain_{F}_lam{lam:.0e}", "ok", chain_spd(F, lam, 3000 + F))
    for name, (P, n) in tile_patterns().items():
        add(f"pattern_{name}", "ok", pattern_spd(P, n, 4000 + n))

    add("neg_row0", "fail", _neg_diag(70, [0], 1))
    add("neg_row15", "fail", _neg_diag(70, [15], 2))
    add("neg_row16", "fail", _neg_diag(70, [16], 3))
    add("neg_row63", "fail", _neg_diag(130, [63], 4))
    add("neg_row64", "fail", _neg_diag(130, [64], 5))
    add("neg_last_row_n64", "fail", _neg_diag(64, [63], 6))
    add("neg_last_row_n70", "fail", _neg_diag(70, [69], 7))
    add("neg_two_rows_one_tile", "fail", _neg_diag(130, [20, 50], 8))
    A, b = pattern_spd(bordered_pattern(), 482, 9)       # tile 2 is on level 1 (block {1, 2}), tile 3 on level 0 (first of block {3, 4, 5})
    A[2 * NB + 22, 2 * NB + 22] = -1.0
    A[3 * NB + 8, 3 * NB + 8] = -1.0
    add("neg_two_rows_two_levels", "fail", (A, b))
    add("zero_pivot", "fail", _zero_pivot(130, 70, 10))
    for p in (62, 63, 64):
        add(f"minor_{p}_{p + 1}", "fail", _minor(130, p, 11 + p))

    add("nan_off_diagonal", "nonfinite", _put(130, [(80, 10, np.nan)], 20))
    add("nan_diagonal", "nonfinite", _put(130, [(70, 70, np.nan)], 21))
    add("inf_inner_row", "nonfinite", _put(130, [(70, 70, np.inf)], 22))
    add("inf_last_row_n64", "nonfinite", _put(64, [(63, 63, np.inf)], 23))
    add("inf_last_row_n70", "nonfinite", _put(70, [(69, 69, np.inf)], 24))
    return tuple(out)


def ok_cases():
    return [c for c in cases() if c["kind"] == "ok"]


def failing_cases():
    return [c for c in cases() if c["kind"] != "ok"]


def recheck_case():
    """the small SPD system solved after every failing call, on the same context"""
    return random_spd(17, 77)


@functools.lru_cache(maxsize=None)
def truth(name):
    """long-double solution, inverse and cond_inf of a must-succeed case; tile plan of its pattern (computed once per process)"""
    c = next(c for c in cases() if c["name"] == name)
    L, bad, _ = factor(c["A"], LD)
    assert bad < 0, name
    x = backward(L, forward(L, _ld(c["b"])))
    X = forward(L, np.eye(L.shape[0], dtype=LD))
    Ainv = X.T @ X
    return dict(x=x, Ainv=Ainv, cond=cond_inf(c["A"], Ainv), sym=tile_symbolic(tile_pattern(c["A"])))


@functools.lru_cache(maxsize=1)
def yardsticks():
    """(eta, rho) that the FLOAT64 run of this reference reaches at worst over the whole must-succeed list: what plain f64 arithmetic
    gives on these matrices.  Taken over the list, not per case (a single case's value is 0.1 to 1.2 units of 2^-53: too noisy to scale)."""
    e = r = 0.0
    for c in ok_cases():
        x, bad = solve(c["A"], c["b"], np.float64)
        assert bad < 0, c["name"]
        X, _ = inverse(c["A"], np.float64)
        e = max(e, eta(c["A"], x, c["b"]))
        r = max(r, rho(c["A"], X))
    return e, r


MARGIN = 4.0     # another summation order (MFMA accumulation chains, FMA, dd * rsqrt(dd)): the margin of tests/test_pnp_cpu.py and tests/test_twoview_cpu.py
