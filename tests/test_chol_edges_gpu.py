"""The Cholesky family of dense_chol.hip — dense solve, planned dense solve (tile plan), tile-sparse level-scheduled solve, explicit inverse — against the
long-double reference of tests/chol_reference.py, on its case list: sizes around every block edge (1, 2, 15/16/17, 47/48/49, 63/64/65, 127/128/129, 192/193,
257), spectra graded up to kappa = 1e12, the pose graph's chain kron(L_F, I_7) + lambda I up to 518 rows, six tile patterns, and the systems that must fail.

What is asserted, per case and form:
  info == 0; the tile-sparse plan's levels / tiles equal the restated symbolic factorisation;
  solves:   eta(A, x, b) = |b - A x| / (|A| |x| + |b|)  <= 4 x the largest eta the reference's FLOAT64 run reaches over the whole must-succeed list;
  inverse:  rho(A, X) = |A X - I| / (|A| |X|)           <= 4 x the same yardstick of the reference's float64 inverse; X exactly symmetric;
  forward:  |x - x_ld| / |x_ld| <= 2 cond_inf(A) (allowed eta): the standard consequence of the backward bound, cond from the long-double inverse;
  the planned and the plain dense solve return the same bits where the tile pattern is dense;
  must-fail, finite: info == the reference's first failing column + 1 in all four forms, the call returns CCM_OK, and the next call on the same context
  solves an SPD system with info == 0;  non-finite input: never info == 0 beside a NaN / Inf in the output, 1 <= info <= n, and info == the column the
  reference's rule (first pivot not > 0 and finite) names.
The same list runs in a child with CCM_CHOL_DIAG=columns (the column form of the 64 x 64 diagonal tile) and in one with CCM_CHOL_CHAIN=split (the inverse's
three-kernel chain): same assertions; bit identity is asserted between the chain forms only (tests/test_dense_chain_gpu.py establishes it).

4 x: the margin tests/test_pnp_cpu.py and tests/test_twoview_cpu.py give another summation order; the MFMA accumulation chains, the FMAs and dd * rsqrt(dd)
are such differences.  The bounds come from the reference alone, not from what the device returns.

Yardsticks (float64 run of the reference, x86-64): eta 1.29, rho 4.05 units of 2^-53, so the bounds are 5.7e-16 and 1.8e-15.
Device maxima (one MI355X, units of 2^-53; recorded, not used: the bounds above were fixed before the first device run):
  eta   dense and planned solve 1.98 (pattern_one_tile), tile-sparse 1.99 (pattern_one_tile); with CCM_CHOL_DIAG=columns 1.82 (chain_37_lam0e+00) and 1.53
  rho   inverse 3.96 (pattern_two_chains); with CCM_CHOL_DIAG=columns 3.98
  forward error / cond_inf: 3.53 dense, 2.50 tile-sparse (graded_193_k1e+00), against 10.3 allowed
  CCM_CHOL_CHAIN=split returns the fused chain's bits.
Both defects the tests were written to expose showed on the kernels as they were and are fixed: the tile-sparse form reported the
failing column of the earliest LEVEL, not the smallest one (neg_two_rows_two_levels: 201 for 151), and a +inf pivot returned info == 0 with a finite, wrong x."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import chol_reference as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.HAVE_EXTENDED, reason="numpy.longdouble has no 64-bit mantissa on this platform")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "chol_edges_run.py")
_spec = importlib.util.spec_from_file_location("chol_edges_run", SCRIPT)
run = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(run)
assert run.ref is ref          # one case list, one set of cached long-double results
VARIANTS = ("blocked_fused", "columns", "split")


@pytest.fixture(scope="module")
def blocked_fused(ctx):
    assert os.environ.get("CCM_CHOL_CHAIN") != "split" and os.environ.get("CCM_CHOL_DIAG") != "columns"
    return run.run_cases(ctx)


def _child(tmp_path_factory, name, value):
    out = str(tmp_path_factory.mktemp("chol_edges") / f"{value}.npz")
    e = dict(os.environ); e[name] = value
    r = subprocess.run([sys.executable, SCRIPT, out], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def columns(tmp_path_factory):
    return _child(tmp_path_factory, "CCM_CHOL_DIAG", "columns")


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    return _child(tmp_path_factory, "CCM_CHOL_CHAIN", "split")


@pytest.fixture
def res(request):
    return request.getfixturevalue(request.param)


_memo = {}


def _measure(kind, case, X):
    """eta or rho of a device result, in long double; computed once per distinct result (the split child returns the fused chain's bits)"""
    key = (kind, case["name"], X.tobytes())
    if key not in _memo:
        _memo[key] = ref.eta(case["A"], X, case["b"]) if kind == "eta" else ref.rho(case["A"], X)
    return _memo[key]


@pytest.mark.parametrize("res", VARIANTS, indirect=True)
def test_every_spd_case_factors_and_the_tile_plan_is_the_symbolic_one(res):
    bad = []
    for c in ref.ok_cases():
        for form in run.FORMS:
            if res[f"{form}__{c['name']}__info"] != 0: bad.append((form, c["name"], int(res[f"{form}__{c['name']}__info"])))
        sym = ref.truth(c["name"])["sym"]
        got = (int(res[f"tile__{c['name']}__levels"]), int(res[f"tile__{c['name']}__tiles"]))
        if got != (sym["levels"], sym["tiles"]): bad.append(("plan", c["name"], got, (sym["levels"], sym["tiles"])))
    assert not bad, bad


@pytest.mark.parametrize("form", run.SOLVES)
@pytest.mark.parametrize("res", VARIANTS, indirect=True)
def test_solve_backward_and_forward_error(res, form, request):
    yard, _ = ref.yardsticks()
    allowed = ref.MARGIN * yard
    bad, worst, worst_fwd = [], (0.0, ""), (0.0, "")
    for c in ref.ok_cases():
        x = res[f"{form}__{c['name']}__x"]
        t = ref.truth(c["name"])
        e = _measure("eta", c, x)
        worst = max(worst, (e, c["name"]))
        if not (np.isfinite(x).all() and e <= allowed): bad.append(("eta", c["name"], e / ref.U53))
        x_ld = t["x"]
        fwd = float(ref.norm_inf(x.astype(ref.LD) - x_ld) / ref.norm_inf(x_ld))
        worst_fwd = max(worst_fwd, (fwd / t["cond"], c["name"]))
        if not fwd <= 2 * t["cond"] * allowed: bad.append(("forward", c["name"], fwd, t["cond"]))
    print(f"\nMEASURED {request.node.callspec.id}: yardstick eta {yard / ref.U53:.3f} u, allowed {allowed / ref.U53:.3f} u, device max eta "
          f"{worst[0] / ref.U53:.3f} u at {worst[1]}, max forward / cond {worst_fwd[0] / ref.U53:.3f} u at {worst_fwd[1]}")
    assert not bad, bad


@pytest.mark.parametrize("res", VARIANTS, indirect=True)
def test_inverse_residual_and_symmetry(res, request):
    _, yard = ref.yardsticks()
    allowed = ref.MARGIN * yard
    bad, worst = [], (0.0, "")
    for c in ref.ok_cases():
        X = res[f"inverse__{c['name']}__x"]
        if not np.array_equal(X, X.T): bad.append(("symmetry", c["name"]))
        r = _measure("rho", c, X)
        worst = max(worst, (r, c["name"]))
        if not (np.isfinite(X).all() and r <= allowed): bad.append(("rho", c["name"], r / ref.U53))
    print(f"\nMEASURED {request.node.callspec.id}: yardstick rho {yard / ref.U53:.3f} u, allowed {allowed / ref.U53:.3f} u, device max rho "
          f"{worst[0] / ref.U53:.3f} u at {worst[1]}")
    assert not bad, bad


@pytest.mark.parametrize("res", VARIANTS, indirect=True)
def test_planned_solve_has_the_dense_solve_s_bits_on_dense_patterns(res):
    n_dense = 0
    for c in ref.ok_cases():
        sym = ref.truth(c["name"])["sym"]
        T = sym["fill"].shape[0]
        if not np.tril(ref.tile_pattern(c["A"])).sum() == T * (T + 1) // 2: continue
        n_dense += 1
        assert np.array_equal(res[f"planned__{c['name']}__x"], res[f"dense__{c['name']}__x"]), c["name"]
    assert n_dense >= 30          # the 17 sizes and the 13 graded spectra, at least


def test_split_chain_has_the_fused_chain_s_bits(blocked_fused, split):
    for c in ref.ok_cases():
        for form in run.FORMS:
            assert np.array_equal(blocked_fused[f"{form}__{c['name']}__x"], split[f"{form}__{c['name']}__x"]), (form, c["name"])


@pytest.mark.parametrize("res", VARIANTS, indirect=True)
@pytest.mark.parametrize("name", [c["name"] for c in ref.failing_cases()])
def test_failing_pivot_report(res, name):
    c = next(c for c in ref.cases() if c["name"] == name)
    n = c["A"].shape[0]
    col = ref.first_failing_pivot(c["A"])
    assert 0 <= col < n
    Ar, br = ref.recheck_case()
    yard, yard_inv = ref.yardsticks()
    for form in run.FORMS:
        info = int(res[f"{form}__{name}__info"])          # the wrapper raised unless the call returned CCM_OK
        out = res[f"{form}__{name}__x"]
        if c["kind"] == "nonfinite":
            assert (info != 0 and 1 <= info <= n) or np.isfinite(out).all(), (form, info)
        assert info == col + 1, (form, info, col + 1)
        # the next call on the same context
        assert res[f"{form}__{name}__re_info"] == 0, form
        if form == "inverse": assert ref.rho(Ar, res[f"{form}__{name}__re_x"]) <= ref.MARGIN * yard_inv
        else: assert ref.eta(Ar, res[f"{form}__{name}__re_x"], br) <= ref.MARGIN * yard
