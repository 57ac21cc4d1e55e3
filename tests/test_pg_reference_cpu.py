"""CPU: pins tests/pg_reference.py (the yardstick of tests/test_posegraph_pcg_gpu.py) on the oracle's own system (oracle.pose_graph_system) before
the device is compared with it: the O(F) forest elimination against the dense inverse of the forest matrix, T positive definite, and the iteration
counts of both preconditioners (lambda = 1e-16, rel_tol = 1e-10, the product's values) at 40 / 120 / 300 keyframes: forest 63 / 73 / 85, block-Jacobi
92 / 269 / 840 in the study that preceded these tests."""
import functools

import numpy as np
import pytest

from ccm_slam_amd import synth
from tests import pg_reference as ref
from tests.test_posegraph_gpu import _concat_graphs

LAM, TOL = 1e-16, 1e-10
LD = np.longdouble


def _graph(name):
    if name.startswith("chain"):                     # chain<n>[s]: one fixed vertex, s = fix_scale
        fs = name.endswith("s")
        return synth.make_pose_graph(int(name[5:].rstrip("s")), 1, fix_scale=fs)
    if name.startswith("fixed3_"):                   # three fixed vertices, two of them neighbours
        n = int(name[7:])
        pg = synth.make_pose_graph(n, 1)
        pg["fixed"] = pg["fixed"].copy()
        pg["fixed"][[n // 2, n // 2 + 1]] = 1
        return pg
    if name.startswith("float_"):                    # a component with a fixed vertex and one without
        n = int(name[6:])
        a, b = synth.make_pose_graph(n, 1), synth.make_pose_graph(12, 2)
        b["fixed"] = np.zeros(12, np.uint8)
        return _concat_graphs([a, b])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _system(name):
    import oracle
    oracle.build()
    pg = _graph(name)
    H, b, J = oracle.pose_graph_system(pg)
    return pg, H, b, J


@pytest.mark.parametrize("name", ["chain12", "chain40", "chain120", "chain12s", "chain40s", "chain120s", "fixed3_12", "fixed3_40", "fixed3_120",
                                  "float_12", "float_40", "float_120"])
def test_forest_elimination_is_the_inverse_of_the_forest_matrix(name):
    """T Z = I in long double for Z = forest_solve(I): the residual is bounded by (long-double epsilon 1.1e-19) x cond(T) (below 1e8 on these graphs,
    asserted) x a small constant, so 1e-9 leaves two orders of room and still catches any structural slip (those give O(1)); and Z equals numpy's f64
    inverse of T within 1e-16 x cond(T) <= 1e-7 of its largest entry."""
    pg, H, b, J = _system(name)
    F = H.shape[0] // 7
    T = ref.forest_matrix(pg, H, J, LAM, LD)
    T64 = T.astype(np.float64)
    assert np.array_equal(T, T.T) or np.abs(T - T.T).max() <= 1e-18 * np.abs(T).max()
    w = np.linalg.eigvalsh(T64)
    assert w[0] > 0, w[0]                                                  # T is SPD
    assert w[-1] / w[0] < 1e8
    cols = np.unique(np.concatenate([np.arange(0, 7 * F, 37), np.arange(7 * F - 7, 7 * F)]))   # a spread of unit vectors and the whole last vertex
    I = np.eye(7 * F)[:, cols]
    Z = ref.forest_solve(pg, H, J, LAM, LD)(I)
    assert np.abs(T @ Z - I).max() < 1e-9
    Zi = np.linalg.inv(T64)
    assert np.abs(Z.astype(np.float64) - Zi[:, cols]).max() <= 1e-7 * np.abs(Zi).max()
    # the f64 run of the same elimination (what the GPU tests measure their bar with) is within f64 epsilon x cond(T) of it
    Z64 = ref.forest_solve(pg, H, J, LAM, np.float64)(I)
    assert np.abs(Z64 - Z).max() <= 1e-7 * np.abs(Zi).max()


def test_forest_has_the_expected_shape():
    pg, H, b, J = _system("float_40")
    tree, roots = ref.forest(pg)
    assert roots == [39]                                                   # first free slot of the second component
    assert len(tree) == 39 + 11                                            # F - (floating components) edges: 39 free + 12 free - 1
    pg, H, b, J = _system("fixed3_40")
    tree, roots = ref.forest(pg)
    assert roots == [] and len(tree) == 37
    assert all(abs(int(pg["e_i"][e]) - int(pg["e_j"][e])) == 1 for e in tree)   # Kruskal by |i - j| on a chain keeps the odometry edges


@functools.lru_cache(maxsize=None)
def _iterations(name, precond, dtype):
    """One reference run: the PCG itself in float64 (as on the device), the preconditioner's reference in `dtype` and rounded to float64"""
    pg, H, b, J = _system(name)
    blocks, keys = ref.blocks_of_dense(H)
    Av = lambda v: ref.matvec(blocks, keys, LAM, v)
    if precond == "forest":
        Md = ref.forest_solve(pg, H, J, LAM, dtype)
    else:
        Md = ref.block_jacobi(H, LAM, dtype)
    M = lambda r: np.asarray(Md(r), np.float64)
    F = H.shape[0] // 7
    x, k, flags = ref.pcg(Av, b, M, TOL, min(50000, 70 * F + 100), precond == "forest")
    res = np.linalg.norm(Av(x) - b) / np.linalg.norm(b)
    return k, flags, res


def test_forest_iterations_do_not_grow_with_the_chain():
    k = {n: _iterations(f"chain{n}", "forest", np.float64)[0] for n in (40, 120, 300)}
    print("forest iterations", k)
    for n in (40, 120, 300):
        kk, flags, res = _iterations(f"chain{n}", "forest", np.float64)
        assert flags[0] == 1 and flags[2] == 0 and flags[3] == 0, (n, flags)
        assert res < 1e-6, (n, res)
        assert k[40] / 1.5 <= kk <= 1.5 * k[40], k


def test_jacobi_iterations_grow_with_the_chain():
    k40, f40, r40 = _iterations("chain40", "jacobi", np.float64)
    k120, f120, r120 = _iterations("chain120", "jacobi", np.float64)
    print("jacobi iterations", k40, k120)
    assert f40[0] == 1 and f120[0] == 1 and f40[2] == 0 and f120[2] == 0
    assert r40 < 1e-8 and r120 < 1e-8
    assert k120 > 2 * k40, (k40, k120)


@pytest.mark.parametrize("name,precond", [("chain40", "forest"), ("chain120", "forest"), ("chain120s", "forest"), ("chain300", "forest"),
                                          ("chain40", "jacobi"), ("chain120", "jacobi"), ("chain120s", "jacobi")])
def test_f64_and_long_double_runs_take_the_same_iterations(name, precond):
    """The reference is run twice, with its preconditioner (forest_solve / block_jacobi) in float64 and in long double, the only place where
    tests/pg_reference.py uses long double; the PCG recurrences are float64 both times, like the device's.  Bar: 2 iterations.  (A run with the
    recurrences in long double as well is a different experiment: it ends 3 ... 8 iterations earlier on the forest cases from chain120 on,
    because the last decade before r.z <= 1e-20 r0.z0 is rounding-limited in float64; DESIGN.md 4.3 records it, no test uses it.)  tests/test_posegraph_pcg_gpu.py computes the same pair on the device's systems."""
    k64 = _iterations(name, precond, np.float64)[0]
    kld = _iterations(name, precond, LD)[0]
    print(name, precond, k64, kld)
    assert abs(k64 - kld) <= 2, (k64, kld)
