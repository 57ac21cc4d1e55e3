"""Essential-graph optimisation on the device (ccm_pose_graph_optimize) vs the oracle restatement of what
Optimizer::OptimizeEssentialGraph{LoopClosure,MapFusion} hand to g2o (oracle/ba_ref.cpp: ora_pose_graph_optimize).

Tolerance: f64 LM with numerically differentiated 7x7 Jacobians (delta 1e-9 amplifies rounding by 5e8); the linear solve is exact on both
sides (device: tile-sparse Cholesky over a nested-dissection order; oracle: block Cholesky in natural order), so only rounding differs.  The LM iteration
and trial COUNTS are compared up to 2000 keyframes (they agree there); near convergence the accept / reject decision of a trial can depend on differences
of rounding size, which is what happens at 10 000 keyframes — no count is asserted at that size.  The optimised Sim3s must agree to 1e-5
(rotation / scale) and 1e-5 m, the final chi2 to 1e-6 of the initial chi2."""
import numpy as np
import pytest

from ccm_slam_amd import optimizer, synth

pytestmark = pytest.mark.gpu


def _check(ctx, oracle_lib, pg):
    s, st = optimizer.pose_graph_optimization(ctx, pg)
    so, sto = oracle_lib.pose_graph_optimize(pg)
    assert st.chi2_initial == pytest.approx(sto.chi2_initial, rel=1e-9)
    assert abs(st.chi2_final - sto.chi2_final) <= 1e-6 * sto.chi2_initial
    assert st.chi2_final < 0.2 * st.chi2_initial                       # the loop error was distributed
    assert np.abs(s - so).max() < 1e-5, np.abs(s - so).max()
    assert np.array_equal(s[pg["fixed"] == 1], pg["sim3"][pg["fixed"] == 1])   # fixed vertices untouched, bit for bit
    assert (st.iters_done, st.lm_trials) == (sto.iters_done, sto.lm_trials)      # same LM path: iterations and trials (sizes up to 2000 keyframes)
    return s, st


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("n_kf,seed", [(40, 0), (120, 1)])
def test_pose_graph_matches_oracle(ctx, oracle_lib, n_kf, seed, fix_scale):
    pg = synth.make_pose_graph(n_kf, seed, fix_scale=fix_scale)
    s, st = _check(ctx, oracle_lib, pg)
    if fix_scale:
        assert np.array_equal(s[:, 7], pg["sim3"][:, 7])               # update[6] is zeroed: scales never move


def test_pose_graph_of_the_bench_workload_matches_oracle(ctx, oracle_lib):
    """bench.py's essential-graph leg: 2000 keyframes / ~10 000 Sim3 edges (covisibility 6), the map size of BASELINE config 4.  Same LM iterations and
    trials as the oracle (2 / 11), Sim3s within 1e-5 (measured 4e-6)."""
    pg = synth.make_pose_graph(2000, 0, covis=6)
    s, st = _check(ctx, oracle_lib, pg)
    assert st.iters_done >= 2


def test_consistent_graph_is_a_fixed_point(ctx):
    pg = synth.make_pose_graph(60, 3, n_loop=0)                        # only drift-consistent edges: error is zero at the start
    s, st = optimizer.pose_graph_optimization(ctx, pg)
    assert st.chi2_initial < 1e-20 and st.chi2_final <= st.chi2_initial
    assert np.abs(s - pg["sim3"]).max() < 1e-9


def test_all_fixed_or_no_edges_is_a_no_op(ctx):
    pg = synth.make_pose_graph(10, 4)
    pg2 = dict(pg); pg2["fixed"] = np.ones(10, np.uint8)
    s, st = optimizer.pose_graph_optimization(ctx, pg2)
    assert st.iters_done == 0 and np.array_equal(s, pg["sim3"])
    pg3 = dict(pg); pg3["e_i"] = pg["e_i"][:0]; pg3["e_j"] = pg["e_j"][:0]; pg3["meas"] = pg["meas"][:0]
    s, st = optimizer.pose_graph_optimization(ctx, pg3)
    assert st.iters_done == 0 and np.array_equal(s, pg["sim3"])


def test_bad_edge_index_is_rejected(ctx):
    pg = synth.make_pose_graph(10, 5)
    pg["e_j"] = pg["e_j"].copy(); pg["e_j"][2] = 99
    with pytest.raises(Exception):
        optimizer.pose_graph_optimization(ctx, pg)


@pytest.mark.parametrize("n", [7, 64, 100, 257, 1000])
def test_dense_mfma_cholesky_solves_spd_systems(ctx, n):
    """The blocked f64 Cholesky behind the pose-graph solve (dense_chol.hip: 64x64 tiles on v_mfma_f64_16x16x4) against
    numpy on random SPD matrices; sizes cover a single partial tile, exact tiles and several tile rows with padding."""
    rng = np.random.default_rng(n)
    M = rng.normal(size=(n, n))
    A = M @ M.T + n * np.eye(n)
    b = rng.normal(size=n)
    x, info = optimizer.debug_dense_solve(ctx, A, b)
    assert info == 0
    ref = np.linalg.solve(A, b)
    assert np.abs(x - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max()) * n


def _spd_with_pattern(n, mask, seed):
    rng = np.random.default_rng(seed)
    M = rng.normal(size=(n, n)) * mask
    A = M + M.T
    A += np.diag(np.abs(A).sum(axis=1) + 1.0)      # diagonally dominant => SPD
    return A, rng.normal(size=n)


@pytest.mark.parametrize("kind,n", [("dense", 200), ("banded", 1000), ("bordered", 900), ("one_tile", 40)])
def test_tile_sparse_level_scheduled_cholesky(ctx, kind, n):
    """ccm_tsc (what ccm_pose_graph_optimize factors with): compact non-zero tiles, left-looking gathers, all tile columns of an elimination
    level per launch.  Dense: one column per level; banded: a chain; bordered block-diagonal (nested-dissection shape): the diagonal blocks
    share levels, i.e. FEWER levels than tile columns."""
    idx = np.arange(n)
    if kind in ("dense", "one_tile"): mask = np.ones((n, n))
    elif kind == "banded": mask = (np.abs(idx[:, None] - idx[None, :]) <= 90).astype(float)
    else:
        blk = np.minimum(idx // 192, 3)                # four diagonal blocks of three tiles, then a border
        border = idx >= 768
        mask = ((blk[:, None] == blk[None, :]) | border[:, None] | border[None, :]).astype(float)
    A, b = _spd_with_pattern(n, mask, n)
    x, info, levels, tiles = optimizer.debug_tile_solve(ctx, A, b)
    assert info == 0
    ref = np.linalg.solve(A, b)
    assert np.abs(x - ref).max() <= 1e-11 * max(1.0, np.abs(ref).max()) * n
    T = (n + 63) // 64
    if kind == "dense": assert levels == T and tiles == T * (T + 1) // 2
    if kind == "banded": assert levels == T and tiles < T * (T + 1) // 2
    if kind == "bordered": assert levels == 3 + (T - 12) and tiles == 4 * 6 + (T - 12) * 12 + (T - 12) * (T - 11) // 2


def test_tile_cholesky_reports_a_non_positive_pivot(ctx):
    A = np.eye(200); A[140, 140] = -1.0
    x, info, _, _ = optimizer.debug_tile_solve(ctx, A, np.ones(200))
    assert info == 141


def test_pose_graph_nested_dissection_matches_the_natural_order_solver(ctx, monkeypatch):
    """500 keyframes: the default exact solver (nested-dissection order, tile-sparse level-scheduled Cholesky) against the round-1 form
    (natural order, dense array, column after column): same LM iterations and trials, Sim3s within 1e-7."""
    pg = synth.make_pose_graph(500, 2, covis=6)
    s1, st1 = optimizer.pose_graph_optimization(ctx, pg)
    monkeypatch.setenv("CCM_PG_SOLVER", "dense")
    s0, st0 = optimizer.pose_graph_optimization(ctx, pg)
    assert (st1.iters_done, st1.lm_trials) == (st0.iters_done, st0.lm_trials)
    assert np.abs(s1 - s0).max() < 1e-7, np.abs(s1 - s0).max()


def _concat_graphs(parts):
    off = 0
    out = dict(sim3=[], fixed=[], e_i=[], e_j=[], meas=[])
    for g in parts:
        out["sim3"].append(g["sim3"]); out["fixed"].append(g["fixed"]); out["meas"].append(g["meas"])
        out["e_i"].append(g["e_i"] + off); out["e_j"].append(g["e_j"] + off)
        off += g["n_vert"]
    r = {k: np.concatenate(v) for k, v in out.items()}
    r.update(fix_scale=False, n_vert=off, n_edge=int(r["e_i"].size))
    return r


def _hub_graph():
    """25 independent 12-keyframe loops (each with its own fixed keyframe), plus a 150-keyframe loop whose vertex 5 also has an edge to every 7th keyframe"""
    parts = [synth.make_pose_graph(12, 100 + k, n_loop=1, covis=2) for k in range(25)]
    big = synth.make_pose_graph(150, 7)
    hub_i, hub_j, hub_m = [], [], []
    for k in range(12, 150, 7):   # consistent extra edges (measured from the drifted estimate): zero error, but they shape the graph
        hub_i.append(k); hub_j.append(5)
        a, b = big["sim3"][5], big["sim3"][k]
        Ra, Rb = synth.R_from_quat(a[None, :4])[0], synth.R_from_quat(b[None, :4])[0]
        Rji = Ra @ Rb.T
        sji = a[7] / b[7]
        tji = a[4:7] - sji * (Rji @ b[4:7])
        hub_m.append(np.concatenate([synth.quat_from_R(Rji[None])[0], tji, [sji]]))
    big = dict(big, e_i=np.concatenate([big["e_i"], np.array(hub_i, np.int32)]), e_j=np.concatenate([big["e_j"], np.array(hub_j, np.int32)]),
               meas=np.concatenate([big["meas"], np.stack(hub_m)]))
    big["n_edge"] = int(big["e_i"].size)
    return _concat_graphs(parts + [big])


def test_disconnected_components_and_a_hub(ctx, oracle_lib):
    """Shapes the nested-dissection order must not choke on: 25 independent 12-keyframe loops (each with its own fixed keyframe: small
    components share pieces), plus a 150-keyframe loop whose vertex 5 also has an edge to every 7th keyframe (a hub: wide BFS levels)."""
    _check(ctx, oracle_lib, _hub_graph())


def test_dense_cholesky_reports_a_non_positive_pivot(ctx):
    A = np.eye(70); A[40, 40] = -1.0
    x, info = optimizer.debug_dense_solve(ctx, A, np.ones(70))
    assert info == 41


@pytest.mark.parametrize("n", [30, 64, 65, 200, 375, 756, 1878])   # 1878 = the coarse operator of the 10 000-keyframe map: 30 tile rows
def test_dense_inverse_tiles(ctx, n):
    rng = np.random.default_rng(n)
    M = rng.normal(size=(n, n))
    A = M @ M.T + n * np.eye(n)
    Ai, info = optimizer.debug_dense_inverse(ctx, A)
    assert info == 0
    assert np.abs(Ai @ A - np.eye(n)).max() < 1e-10
    assert np.abs(Ai - Ai.T).max() == 0.0      # mirrored tiles: exactly symmetric
