"""The dense inverse's fused launch chain (dense_chol.hip: diagonal tile, then ONE launch with the panel, the trailing update and the previous L^-1 step)
against the split chain it replaces (diagonal tile / panel / update, the L^-1 steps afterwards; CCM_CHOL_CHAIN=split).  Both run the same MFMA sequences on the
same operands per tile, so every result is compared with np.array_equal, not to a tolerance.  The switch is read once per process: the split form runs in a
child (scripts/dense_chain_run.py), once for all sizes.

What the split switch does NOT move: the dense solve (debug_dense_solve) and the tile-sparse solve (debug_tile_solve) keep their launch lists, and the 64 x 64
diagonal body (phase (a) now runs ahead on a third wave) is the same in both processes.  That body is pinned by recorded results of the parent commit instead
(test_results_have_the_bits_of_the_commit_before_the_fused_chain)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "scripts", "dense_chain_run.py")
_spec = importlib.util.spec_from_file_location("dense_chain_run", SCRIPT)
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)


@pytest.fixture(scope="module")
def fused(ctx):
    assert os.environ.get("CCM_CHOL_CHAIN") != "split"
    return cases.run_cases(ctx)


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dense_chain") / "split.npz")
    e = dict(os.environ); e["CCM_CHOL_CHAIN"] = "split"
    r = subprocess.run([sys.executable, SCRIPT, out], env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return dict(np.load(out))


@pytest.mark.parametrize("n", cases.SIZES)
def test_fused_chain_has_the_split_chain_s_bits(fused, split, n):
    assert fused[f"ainv_info_{n}"] == 0 and split[f"ainv_info_{n}"] == 0
    assert np.array_equal(fused[f"ainv_{n}"], split[f"ainv_{n}"])
    assert fused[f"x_info_{n}"] == 0 and split[f"x_info_{n}"] == 0
    assert np.array_equal(fused[f"x_{n}"], split[f"x_{n}"])


@pytest.mark.parametrize("n", cases.SIZES)
def test_inverse_is_exactly_symmetric_and_an_inverse(fused, n):
    A, _ = cases.spd(n)
    Ai = fused[f"ainv_{n}"]
    assert np.array_equal(Ai, Ai.T)
    assert np.abs(Ai @ A - np.eye(n)).max() < 1e-10   # bound of tests/test_posegraph_gpu.py::test_dense_inverse_tiles


@pytest.mark.parametrize("n,row", cases.PIVOTS)
def test_non_positive_pivot_is_reported(fused, split, n, row):
    for res in (fused, split):
        assert res[f"pivot_inv_{n}"] == row + 1
        assert res[f"pivot_solve_{n}"] == row + 1


def test_results_have_the_bits_of_the_commit_before_the_fused_chain(fused, split):
    """tests/golden/dense_chain_parent.npz: what the parent commit's library (split chain, phase (a) of the diagonal tile on the pivot wave alone) returned for
    the two integer-valued cases of scripts/dense_chain_run.py on an MI355X.  The tile-sparse solve shares only the 64 x 64 diagonal body with the inverse."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "dense_chain_parent.npz"))
    for res in (fused, split):
        assert res["tile_info"] == 0 and res["gold_ainv_info"] == 0
        assert np.array_equal(res["tile_x"], gold["tile_x"])
        assert np.array_equal(res["gold_ainv"], gold["gold_ainv"])
    A, b = cases.tile_case()
    ref = np.linalg.solve(A, b)
    assert np.abs(fused["tile_x"] - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max()) * b.size
