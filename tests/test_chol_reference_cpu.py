"""CPU: tests/chol_reference.py checked against itself and against closed forms, so that tests/test_chol_edges_gpu.py measures the device with a
yardstick that is known to be right: every must-succeed case is comfortably factorable in f64, the long-double factor reproduces A to a few units
of 2^-64, the restated symbolic tile factorisation gives the closed-form level and tile counts, and the first-failing-pivot report names the
planted columns."""
import numpy as np
import pytest

from tests import chol_reference as ref

pytestmark = pytest.mark.skipif(not ref.HAVE_EXTENDED, reason="numpy.longdouble has no 64-bit mantissa on this platform")

U64 = 2.0 ** -64


def test_case_list_is_what_the_issue_names():
    names = [c["name"] for c in ref.cases()]
    assert len(names) == len(set(names))
    ok = ref.ok_cases()
    assert sorted(c["A"].shape[0] for c in ok if c["name"].startswith("spd_")) == list(ref.SIZES)
    assert len([c for c in ok if c["name"].startswith("graded_")]) == 13 and len([c for c in ok if c["name"].startswith("chain_")]) == 8
    assert sorted(c["A"].shape[0] for c in ok if c["name"].startswith("chain_")) == [63, 63, 70, 70, 259, 259, 518, 518]
    assert len([c for c in ok if c["name"].startswith("pattern_")]) == 6
    for c in ref.cases():
        A = c["A"]
        assert A.shape[0] <= ref.MAX_ROWS and A.shape == (c["b"].size,) * 2
        assert np.array_equal(A, A.T, equal_nan=True)


def test_every_must_succeed_case_is_comfortably_factorable_in_f64():
    """no failing pivot in the float64 run, and the smallest pivot is at least 100 n u |A|_inf (measured: 2.0e-11 against 5.7e-12 at
    graded n = 193, kappa = 1e12, the tightest case)"""
    for c in ref.ok_cases():
        A = c["A"]
        n = A.shape[0]
        L, bad, dmin = ref.factor(A, np.float64)
        assert bad == -1, c["name"]
        assert dmin >= 100 * n * ref.U53 * float(ref.norm_inf(A)), (c["name"], dmin)


def test_long_double_factor_reproduces_the_matrix():
    """|L L^T - A| <= (n + 1) u64 |L| |L|^T elementwise bounds the factorisation (Higham, Thm 10.3); measured: at most 1.7 units of 2^-64 |A|_inf"""
    for c in ref.ok_cases():
        A = c["A"].astype(ref.LD)
        L, bad, _ = ref.factor(c["A"], ref.LD)
        assert bad == -1
        err = float(ref.norm_inf(L @ L.T - A) / ref.norm_inf(A))
        assert err <= 4 * U64, (c["name"], err / U64)


def test_solve_and_inverse_in_long_double():
    for name in ("spd_65", "graded_129_k1e+08", "chain_37_lam0e+00"):
        c = next(c for c in ref.cases() if c["name"] == name)
        t = ref.truth(name)
        assert ref.eta(c["A"], t["x"].astype(np.float64), c["b"]) <= 2 * ref.U53       # rounding x to f64 is all that is left
        n = c["A"].shape[0]
        R = c["A"].astype(ref.LD) @ t["Ainv"] - np.eye(n, dtype=ref.LD)
        assert float(ref.norm_inf(R)) <= 64 * n * U64 * t["cond"]
        assert np.array_equal(t["Ainv"], t["Ainv"].T)
    A = np.array([[4.0, 2.0], [2.0, 5.0]])
    x, bad = ref.solve(A, np.array([2.0, 9.0]), np.float64)
    assert bad == -1 and np.allclose(x, [-0.5, 2.0], rtol=0, atol=1e-15)
    Ai, _ = ref.inverse(A, np.float64)
    assert np.allclose(Ai, np.array([[5.0, -2.0], [-2.0, 4.0]]) / 16, rtol=0, atol=1e-16)


def test_yardsticks_are_a_few_units_of_f64_roundoff():
    """measured on x86-64: eta 1.29, rho 4.05 units of 2^-53"""
    e, r = ref.yardsticks()
    assert 0.25 * ref.U53 <= e <= 8 * ref.U53
    assert 0.25 * ref.U53 <= r <= 16 * ref.U53


def _tiles_formula(kind, T):
    if kind == "dense": return T, T * (T + 1) // 2
    if kind == "bordered": return 3 + (T - 12), 4 * 6 + (T - 12) * 12 + (T - 12) * (T - 11) // 2


def test_symbolic_restatement_gives_the_formulas_the_tile_sparse_test_asserts():
    """the three levels / tiles statements of tests/test_posegraph_gpu.py::test_tile_sparse_level_scheduled_cholesky, on its own masks"""
    def pattern(n, mask):
        return ref.tile_pattern(mask.astype(float) + np.eye(n))
    n = 200; T = 4
    s = ref.tile_symbolic(pattern(n, np.ones((n, n))))
    assert (s["levels"], s["tiles"]) == _tiles_formula("dense", T)
    n = 1000; T = 16; idx = np.arange(n)
    s = ref.tile_symbolic(pattern(n, np.abs(idx[:, None] - idx[None, :]) <= 90))
    assert s["levels"] == T and s["tiles"] < T * (T + 1) // 2
    assert s["tiles"] == T + (T - 1) + (T - 2)          # |i - j| <= 90 reaches two tiles down: a band of three tile diagonals, no fill outside it
    n = 900; T = 15; idx = np.arange(n)
    blk = np.minimum(idx // 192, 3); border = idx >= 768
    s = ref.tile_symbolic(pattern(n, (blk[:, None] == blk[None, :]) | border[:, None] | border[None, :]))
    assert (s["levels"], s["tiles"]) == _tiles_formula("bordered", T)
    assert s["level"][:12] == [0, 1, 2] * 4


def test_symbolic_restatement_on_the_listed_patterns():
    sym = {name: ref.tile_symbolic(np.tril(P | np.eye(P.shape[0], dtype=bool))) for name, (P, n) in ref.tile_patterns().items()}
    assert (sym["block_diagonal"]["levels"], sym["block_diagonal"]["tiles"]) == (1, 4)
    assert (sym["wrong_way_arrow"]["levels"], sym["wrong_way_arrow"]["tiles"]) == (6, 21)          # full fill
    assert sym["two_chains"]["level"] == [0, 1, 2, 0, 1, 2, 3, 4] and sym["two_chains"]["tiles"] == 14
    assert sym["bordered_unequal"]["level"] == [0, 0, 1, 0, 1, 2, 3, 4] and sym["bordered_unequal"]["tiles"] == 1 + 3 + 6 + 2 * 6 + 3
    assert (sym["one_tile"]["levels"], sym["one_tile"]["tiles"]) == (1, 1)
    # fill is a superset of the pattern and closed under elimination: (i, j), (k, j) in L with i > k > j => (i, k) in L
    for name, (P, n) in ref.tile_patterns().items():
        F = sym[name]["fill"]; T = F.shape[0]
        assert (F | np.tril(P)).sum() == F.sum()
        for j in range(T):
            rows = [i for i in range(j + 1, T) if F[i, j]]
            assert all(F[a, b] for a in rows for b in rows if a > b)
    # the pattern of the matrices themselves is the listed one
    for c in ref.ok_cases():
        if c["name"].startswith("pattern_"):
            P, n = ref.tile_patterns()[c["name"][len("pattern_"):]]
            assert np.array_equal(ref.tile_pattern(c["A"]), np.tril(P | P.T | np.eye(P.shape[0], dtype=bool)))
    # the chain is block tridiagonal by tiles
    c = next(c for c in ref.cases() if c["name"] == "chain_74_lam0e+00")
    s = ref.truth(c["name"])["sym"]
    assert (s["levels"], s["tiles"]) == (9, 17)


EXPECTED_BAD = dict(neg_row0=0, neg_row15=15, neg_row16=16, neg_row63=63, neg_row64=64, neg_last_row_n64=63, neg_last_row_n70=69,
                    neg_two_rows_one_tile=20, neg_two_rows_two_levels=2 * 64 + 22, zero_pivot=70, minor_62_63=63, minor_63_64=64, minor_64_65=65,
                    nan_off_diagonal=80, nan_diagonal=70, inf_inner_row=70, inf_last_row_n64=63, inf_last_row_n70=69)


def test_first_failing_pivot_names_the_planted_column_in_both_precisions():
    fails = ref.failing_cases()
    assert sorted(c["name"] for c in fails) == sorted(EXPECTED_BAD)
    for c in fails:
        assert ref.first_failing_pivot(c["A"], ref.LD) == EXPECTED_BAD[c["name"]], c["name"]
        assert ref.first_failing_pivot(c["A"], np.float64) == EXPECTED_BAD[c["name"]], c["name"]
    for c in fails:
        if c["name"].startswith("minor_"):
            assert (np.diag(c["A"]) > 0).all()                       # every diagonal entry is positive: only elimination shows it
    c = next(c for c in fails if c["name"] == "neg_two_rows_two_levels")
    lvl = ref.tile_symbolic(ref.tile_pattern(c["A"]))["level"]
    assert lvl[2] > lvl[3]                                            # the LATER column is on the EARLIER level
    A = np.array([[1.0, 2.0], [2.0, 1.0]])
    assert ref.first_failing_pivot(A) == 1 and ref.first_failing_pivot(np.eye(3)) == -1
    assert ref.first_failing_pivot(np.diag([1.0, 0.0, -1.0])) == 1
