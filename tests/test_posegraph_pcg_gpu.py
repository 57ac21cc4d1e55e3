"""The pose graph's two iterative solve paths on the device (posegraph.hip: PCG with the spanning-forest preconditioner, and block-Jacobi PCG)
through the test hook ccm_debug_pg_solve (one linearisation, one solve of (H + lambda I) x = b by the product's kernels and launch shapes), against
tests/pg_reference.py: plain numpy, float64 and long double.  Every bar is either derivable (the gamma_n bound of a dot product), or a multiple of the
distance between the reference's own float64 and long-double runs, or one of the two rules of tests/test_pcg_one_exchange_gpu.py (true residual
within 10x the reference PCG's, iterations within 2).  DESIGN.md 4.3 records the measured values."""
import functools

import numpy as np
import pytest

from ccm_slam_amd import optimizer, synth
from ccm_slam_amd._lib import CcmError
from tests import pg_reference as ref
from tests.test_posegraph_gpu import _concat_graphs, _hub_graph

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
LAM0, TOL = 1e-16, 1e-10          # the product's lambda_init and rel_tol


# ---- graphs -----------------------------------------------------------------------------------------------------------------------------
def _chain(F, fix_scale=False):
    """chain of F + 1 keyframes with covisibility and loop edges, vertex 0 fixed: F free vertices"""
    n = F + 1
    return synth.make_pose_graph(n, 1, fix_scale=fix_scale, n_loop=3 if n >= 8 else 1)


def _components(floating=()):
    parts = [synth.make_pose_graph(12, 100 + k, n_loop=1, covis=2) for k in range(5)]
    for k in floating:
        parts[k]["fixed"] = np.zeros(12, np.uint8)
    return _concat_graphs(parts)


@functools.lru_cache(maxsize=None)
def _graph(name):
    if name.startswith("chain"):                          # chain<F>[s]
        return _chain(int(name[5:].rstrip("s")), name.endswith("s"))
    pg = synth.make_pose_graph(120, 1)
    if name == "fixed3":
        pg["fixed"] = pg["fixed"].copy(); pg["fixed"][[20, 21]] = 1
    elif name == "fixed_mid":
        pg["fixed"] = np.zeros(120, np.uint8); pg["fixed"][60] = 1
    elif name == "comps5":
        pg = _components()
    elif name == "comps5_float2":
        pg = _components(floating=(1, 3))
    elif name == "hub":
        pg = _hub_graph()
    else:
        raise KeyError(name)
    return pg


FAMILIES = ["chain119", "chain119s", "fixed3", "fixed_mid", "comps5", "comps5_float2", "hub"]
FOREST_F = [1, 2, 7, 127, 128, 129, 300, 2600]          # pg_scan7: 1 -> 2 positions per chunk at 129, empty trailing chunks; 2600 = the LDS limit
JACOBI_D = [1, 31, 32, 33, 255, 256, 257, 300]          # n_wg_upd = ceil(F / 32), n_wg_init = ceil(F / 256)
FOREST_D = [1, 7, 129, 300, 2600]


_HOOK = {}


def _hook(ctx, name, solver, lam_kind="lam0", max_it=None):
    """one hook call per (graph, solver, lambda), shared by the tests; lam_kind: lam0 = 1e-16, diag = 1e-5 max diag(H)"""
    key = (name, solver, lam_kind, max_it)
    if key not in _HOOK:
        pg = _graph(name)
        lam = LAM0
        if lam_kind == "diag":
            H0 = _hook(ctx, name, solver, "lam0", 0)
            lam = 1e-5 * np.abs(np.einsum("kii->ki", H0["H"][:H0["F"]])).max()
        F = int((pg["fixed"] == 0).sum())
        r = optimizer.debug_pg_solve(ctx, pg, lam, solver, TOL, min(50000, 70 * F + 100) if max_it is None else max_it)
        r["lam"] = lam
        _HOOK[key] = r
    return _HOOK[key]


def _full_J(pg, h):
    """the hook's Jacobians indexed like the caller's edge list"""
    J = np.zeros((int(pg["e_i"].size), 2, 7, 7))
    J[h["active"]] = h["J"]
    return J


# ---- a. the system ------------------------------------------------------------------------------------------------------------------------
def _gamma(n):
    return n * U / (1 - n * U)


@pytest.mark.parametrize("name", FAMILIES + ["chain1", "chain2", "chain300"])
def test_h_and_b_are_the_gather_of_the_hooks_own_jacobians(ctx, name):
    """pg_assemble and the host's block / side codes: every H block and b segment recomputed in long double from the hook's own J and err by the gather
    definition (H_ab = sum over the edges joining a and b of Ja^T Jb, rows = the lower slot; b_a = -sum Ja^T err).  Bound: a sum of n products
    evaluated in any order in f64 is within gamma_n sum|x||y| of the exact value, gamma_n = n u / (1 - n u), u = 2^-53; n = 7 (edges in the block) + 2
    covers the 7-term dot product per edge, the sum over edges and the long-double reference's own rounding."""
    pg, h = _graph(name), _hook(ctx, name, "jacobi", "lam0", 0)
    slot = ref.slots(pg)
    keys = {(int(a), int(b)): k for k, (a, b) in enumerate(h["keys"])}
    assert len(keys) == h["nBlk"] and [tuple(k) for k in h["keys"][:h["F"]]] == [(a, a) for a in range(h["F"])]
    nB, F = h["nBlk"], h["F"]
    Hx, Ha, cnt = np.zeros((nB, 7, 7), LD), np.zeros((nB, 7, 7), LD), np.zeros(nB, int)
    bx, ba, bcnt = np.zeros((F, 7), LD), np.zeros((F, 7), LD), np.zeros(F, int)
    J, err = h["J"].astype(LD), h["err"].astype(LD)
    for e, eo in enumerate(h["active"]):
        s = (slot[pg["e_i"][eo]], slot[pg["e_j"][eo]])
        for side in range(2):
            if s[side] >= 0:
                Hx[s[side]] += J[e, side].T @ J[e, side]; Ha[s[side]] += np.abs(J[e, side]).T @ np.abs(J[e, side]); cnt[s[side]] += 1
                bx[s[side]] -= J[e, side].T @ err[e]; ba[s[side]] += np.abs(J[e, side]).T @ np.abs(err[e]); bcnt[s[side]] += 1
            else:
                assert not h["J"][e, side].any()                         # the fixed side has no Jacobian
        if s[0] >= 0 and s[1] >= 0:
            lo, hi = (0, 1) if s[0] < s[1] else (1, 0)
            k = keys[(s[lo], s[hi])]
            Hx[k] += J[e, lo].T @ J[e, hi]; Ha[k] += np.abs(J[e, lo]).T @ np.abs(J[e, hi]); cnt[k] += 1
    assert (cnt > 0).all()                                               # no block without an edge
    gH = np.array([_gamma(7 * c + 2) for c in cnt])[:, None, None]
    gb = np.array([_gamma(7 * c + 2) for c in bcnt])[:, None]
    dH, db = np.abs(h["H"] - Hx), np.abs(h["b"].reshape(F, 7) - bx)
    print(name, "H: worst |diff| / bound", float((dH / np.maximum(gH * Ha, 1e-300)).max()), " b:", float((db / np.maximum(gb * ba, 1e-300)).max()))
    assert (dH <= gH * Ha).all()
    assert (db <= gb * ba).all()


# 10 x the largest distance between the oracle's two builds of the same source (liboracle.so: -O2, no FMA contraction; liboracle_fast.so: -O3
# -march=native with contraction) over the graphs of this test, relative to the largest entry of H resp. b (measured 3.94e-6 / 6.97e-7,
# both on the 301-keyframe chain); for J the largest absolute distance (entries are O(1)): measured 7.07e-6 on the same chain.
# scripts/pg_oracle_spread.py prints the three spreads.
ORACLE_BAR_H, ORACLE_BAR_B, ORACLE_BAR_J = 3.94e-5, 6.97e-6, 7.07e-5


@pytest.mark.parametrize("name", FAMILIES + ["chain1", "chain2", "chain300"])
def test_h_and_b_match_the_oracles_system(ctx, oracle_lib, name):
    """pg_linearize + pg_assemble against oracle.pose_graph_system (the same central differences in scalar C++).  The numeric Jacobian amplifies
    rounding by 1 / (2e-9) = 5e8, so the yardstick is what two builds of the oracle's own source differ by."""
    pg, h = _graph(name), _hook(ctx, name, "jacobi", "lam0", 0)
    Ho, bo, Jo = oracle_lib.pose_graph_system(pg)
    blocks = np.stack([Ho[7 * a:7 * a + 7, 7 * b:7 * b + 7] for a, b in h["keys"]])
    mask = np.zeros((h["F"], h["F"]), bool)
    mask[h["keys"][:, 0], h["keys"][:, 1]] = mask[h["keys"][:, 1], h["keys"][:, 0]] = True
    assert not Ho.reshape(h["F"], 7, h["F"], 7).transpose(0, 2, 1, 3)[~mask].any()          # the device's block list misses no non-zero block
    dH, db = np.abs(h["H"] - blocks).max() / np.abs(Ho).max(), np.abs(h["b"] - bo).max() / max(np.abs(bo).max(), 1e-300)
    dJ = np.abs(h["J"] - Jo[h["active"]]).max()
    print(name, "H", dH, "b", db, "J", dJ)
    assert dH <= ORACLE_BAR_H and db <= ORACLE_BAR_B and dJ <= ORACLE_BAR_J
    assert not Jo[np.setdiff1d(np.arange(Jo.shape[0]), h["active"])].any()                   # edges the device leaves out have no Jacobian in the oracle either


# ---- b. the forest ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES + ["chain1", "chain2", "chain7", "chain129", "chain2600"])
def test_forest_structure(ctx, name):
    pg, h = _graph(name), _hook(ctx, name, "forest", "lam0", 0)
    F = h["F"]
    slot = ref.slots(pg)
    order, pos, out, parent, code = h["t_order"], h["t_pos"], h["t_out"], h["t_parent"], h["t_code"]
    assert sorted(order) == list(range(F))                                # every free vertex once
    assert np.array_equal(pos[order], np.arange(F))
    size = np.ones(F, int)
    for a in order[::-1]:                                                 # children come after their parents, so this sums subtrees
        if parent[a] >= 0:
            assert pos[parent[a]] < pos[a]
            size[parent[a]] += size[a]
    assert np.array_equal(out - pos, size)
    for a in range(F):                                                    # a subtree is the DFS interval [pos, out)
        if parent[a] >= 0:
            assert pos[parent[a]] < pos[a] and out[a] <= out[parent[a]]
    tree, roots = ref.forest(pg)
    edges = []
    for a in range(F):
        if code[a] < 0:
            assert parent[a] == -1 and a in roots
            continue
        e, side = h["active"][code[a] >> 1], code[a] & 1
        ends = (int(pg["e_i"][e]), int(pg["e_j"][e]))
        assert slot[ends[side]] == a                                      # this vertex sits on the side the code says
        other = slot[ends[side ^ 1]]
        assert other == parent[a] if parent[a] >= 0 else (other == -1 and pg["fixed"][ends[side ^ 1]])
        edges.append(int(e))
    assert sorted(edges) == tree
    assert sorted(a for a in range(F) if code[a] < 0) == roots


# ---- c. the preconditioners alone -----------------------------------------------------------------------------------------------------
def _probe_vectors(F, first, last):
    rng = np.random.default_rng(F)
    e0, e1 = np.zeros(7 * F), np.zeros(7 * F)
    e0[7 * first] = 1.0
    e1[7 * last + 6] = 1.0
    return [rng.normal(size=7 * F), e0, e1]


def _lam_kind(name):
    return "diag" if name == "comps5_float2" else "lam0"


@pytest.mark.parametrize("name", [f"chain{F}" for F in FOREST_F] + FAMILIES)
def test_forest_preconditioner_alone(ctx, name):
    """z = M^-1 r of one pg_precond launch (after pg_tree_setup) against the O(F) block elimination of pg_reference.forest_solve in long double, for a
    random r and the unit vectors of the first and the last DFS position.  Bar: 10 x the distance between the reference's float64 and long-double
    runs on the same r."""
    pg = _graph(name)
    h0 = _hook(ctx, name, "forest", _lam_kind(name), 0)
    F, lam = h0["F"], h0["lam"]
    J, Hd = _full_J(pg, h0), h0["H"][:F]
    M64, MLD = ref.forest_solve(pg, Hd, J, lam, np.float64), ref.forest_solve(pg, Hd, J, lam, LD)
    for i, r in enumerate(_probe_vectors(F, h0["t_order"][0], h0["t_order"][-1])):
        z = optimizer.debug_pg_solve(ctx, pg, lam, "forest", TOL, 0, r_in=r)["z"]
        zl = MLD(r)
        bar = 10 * float(np.abs(M64(r) - zl).max())
        d = float(np.abs(z - zl).max())
        print(name, "vector", i, "device - LD", d, "bar", bar, "|z|", float(np.abs(zl).max()))
        assert d <= bar, (name, i, d, bar)


@pytest.mark.parametrize("name", [f"chain{F}" for F in FOREST_F] + FAMILIES)
def test_jacobi_preconditioner_alone(ctx, name):
    """z = blockdiag(H_aa + lambda I)^-1 r of pg_pcg_init against pg_reference.block_jacobi in long double; same vectors and bar as the forest's"""
    pg = _graph(name)
    h0 = _hook(ctx, name, "jacobi", _lam_kind(name), 0)
    F, lam = h0["F"], h0["lam"]
    M64, MLD = ref.block_jacobi(h0["H"][:F], lam, np.float64), ref.block_jacobi(h0["H"][:F], lam, LD)
    for i, r in enumerate(_probe_vectors(F, 0, F - 1)):
        z = optimizer.debug_pg_solve(ctx, pg, lam, "jacobi", TOL, 0, r_in=r)["z"]
        zl = MLD(r)
        bar = 10 * float(np.abs(M64(r) - zl).max())
        d = float(np.abs(z - zl).max())
        print(name, "vector", i, "device - LD", d, "bar", bar, "|z|", float(np.abs(zl).max()))
        assert d <= bar, (name, i, d, bar)


# ---- d. whole solves ------------------------------------------------------------------------------------------------------------------
# The iteration rule: within 2 of the reference's count; where the reference's own float64 / long-double pair differs by more than 2, within that
# spread + 2.  The pair is the one tests/test_pg_reference_cpu.py holds to 2 iterations on the oracle's systems: the PCG recurrences in float64 both
# times (as on the device), the preconditioner's reference (forest_solve / block_jacobi) in float64 and in long double.  It is computed here, on the
# device's own H, b and J (measured: 0 ... 1, but 6 at block-Jacobi F = 256 / 257 / 300 with lambda = 1e-16 or 1e-5 max diag, 3 at fixed3, 5 / 13 on
# the hub graph).
#
# Three named cases get a second allowance, also computed here from the reference alone.  At rel_tol 1e-10 the last decade of r.z is rounding-limited
# in float64, so the count depends on the ORDER of the sums, which is where device (wave butterflies, per-workgroup partials) and numpy (pairwise
# sums) differ.  Re-running the float64 reference with nothing changed but the order of the unknowns inside its dot products moves its own count over
# 588 ... 595 (block-Jacobi F = 255, lambda = 1e-5 max diag H; device 588), 690 ... 696 (F = 300, same lambda; device 685) and 70 ... 73 (fixed_mid
# forest, same lambda; device 73).  For these cases the device is allowed (max - min of the reference's count over the six orders below) + 2.
SUM_ORDER_CASES = {("chain255", "jacobi", "diag"), ("chain300", "jacobi", "diag"), ("fixed_mid", "forest", "diag")}


def _reference_solve(pg, h, solver):
    """float64 reference PCG on the hook's system; also the iteration count with the preconditioner's reference in long double"""
    F, lam = h["F"], h["lam"]
    Av = lambda v: ref.matvec(h["H"], h["keys"], lam, v)
    mk = (lambda dt: ref.forest_solve(pg, h["H"][:F], _full_J(pg, h), lam, dt)) if solver == "forest" else (lambda dt: ref.block_jacobi(h["H"][:F], lam, dt))
    M, max_it = mk(np.float64), min(50000, 70 * F + 100)
    x, k, flags = ref.pcg(Av, h["b"], M, TOL, max_it, solver == "forest")
    k_ld = k
    if not flags[3]:
        Ml = mk(LD)
        k_ld = ref.pcg(Av, h["b"], lambda r: np.asarray(Ml(r), np.float64), TOL, max_it, solver == "forest")[1]
    return x, k, flags, Av, M, k_ld


def _sum_order_spread(Av, b, M, k, max_it, stall):
    """max - min of the float64 reference's iteration count over the natural order and five random orders of the unknowns inside its dot products"""
    ks = [k]
    for seed in range(1, 6):
        p = np.random.default_rng(seed).permutation(b.size)
        ip = np.argsort(p)
        ks.append(ref.pcg(lambda v: Av(v[ip])[p], b[p], lambda r: M(r[ip])[p], TOL, max_it, stall)[1])
    return max(ks) - min(ks), ks


def _check_solve(ctx, name, solver, lam_kind):
    pg = _graph(name)
    h = _hook(ctx, name, solver, lam_kind)
    xr, kr, fr, Av, M, k_ld = _reference_solve(pg, h, solver)
    nb = np.linalg.norm(h["b"])
    res, res_ref = np.linalg.norm(Av(h["x"]) - h["b"]), np.linalg.norm(Av(xr) - h["b"])
    print(name, solver, lam_kind, "lambda", h["lam"], "device flags", h["flags"], "reference", fr, "with long-double preconditioner", k_ld,
          "residual / |b|: device", res / nb, "reference", res_ref / nb)
    assert h["flags"][2] == 0 and fr[2] == 0
    bar = 10 * res_ref + 1e-12 * nb
    assert res <= bar, (res, res_ref)
    if fr[3]:
        assert h["flags"][3] == 1                                         # the reference ended by the stall rule: so must the device
    else:
        assert h["flags"][0] == 1 and h["flags"][3] == 0
        spread = abs(kr - k_ld)
        allowed = spread + 2 if spread > 2 else 2
        if (name, solver, lam_kind) in SUM_ORDER_CASES:
            so, ks = _sum_order_spread(Av, h["b"], M, kr, min(50000, 70 * h["F"] + 100), solver == "forest")
            print(name, solver, lam_kind, "reference counts under other summation orders", ks)
            allowed = max(allowed, so + 2)
        assert abs(int(h["flags"][1]) - kr) <= allowed, (h["flags"], kr, k_ld, allowed)
    return h, Av, bar


@pytest.mark.parametrize("lam_kind", ["lam0", "diag"])
@pytest.mark.parametrize("F", FOREST_D)
def test_forest_pcg_solves(ctx, F, lam_kind):
    """pg_tree_setup, pg_pcg_start, pg_precond, pg_pcg_spmv, pg_pcg_update_xr at rel_tol 1e-10: no failure, true residual <= 10 x the numpy PCG's
    + 1e-12 |b|, iterations within 2 of it (both rules of test_pcg_one_exchange_gpu.py; see _check_solve for the reference pair).  F = 2600 is the largest forest: 153 920 bytes of LDS.
    At F = 2600 and lambda = 1e-5 max diag(H) the reference ends by the stall rule (float64: iteration 138, residual 4.0e-3 |b|; long double: 430,
    6.6e-5) and so does the device (380, 2.4e-4): lambda is not part of the forest matrix, and at this size it exceeds T's smallest eigenvalues.  With
    the product's lambda = 1e-16 the same graph converges in 89 iterations to 4.8e-8 |b| (reference 90)."""
    name = f"chain{F}"
    h, Av, bar = _check_solve(ctx, name, "forest", lam_kind)
    if F == 2600:   # the exact solver of the same hook: it meets the residual rule too, hence the two solutions differ by at most two bars in the A-norm's image
        ht = _hook(ctx, name, "tiles", lam_kind)
        assert ht["flags"][2] == 0
        assert np.array_equal(ht["H"], h["H"]) and np.array_equal(ht["b"], h["b"])
        assert np.linalg.norm(Av(ht["x"]) - h["b"]) <= bar
        assert np.linalg.norm(Av(h["x"] - ht["x"])) <= 2 * bar


@pytest.mark.parametrize("lam_kind", ["lam0", "diag"])
@pytest.mark.parametrize("F", JACOBI_D)
def test_jacobi_pcg_solves(ctx, F, lam_kind):
    """pg_pcg_init, pg_pcg_spmv, pg_pcg_update, forced below the size where the product takes them; same rules"""
    _check_solve(ctx, f"chain{F}", "jacobi", lam_kind)


@pytest.mark.parametrize("solver", ["forest", "jacobi"])
@pytest.mark.parametrize("name", FAMILIES)
def test_pcg_solves_of_the_graph_families(ctx, name, solver):
    lam_kind = _lam_kind(name)       # the floating components are solved at lambda = 1e-5 max diag(H) only, the other families at both
    _check_solve(ctx, name, solver, lam_kind)
    if lam_kind == "lam0":
        _check_solve(ctx, name, solver, "diag")


def test_floating_components_stall_at_the_products_lambda(ctx):
    """Two of five components without a fixed vertex at lambda = 1e-16: the numpy model ends by the stall rule (iteration 72, residual 5.7e-6 |b| in
    float64, 2.7e-6 in long double), and so must the device (measured: iteration 72, 5.6e-6) - the residual rule holds, no failure is flagged."""
    h, Av, bar = _check_solve(ctx, "comps5_float2", "forest", "lam0")
    assert h["flags"][3] == 1


# ---- e. failure flags ---------------------------------------------------------------------------------------------------------------------
def test_failure_flags(ctx):
    """An indefinite system is reported, not solved: lambda = -2 max diag(H) gives a non-positive pivot in pg_pcg_init (Jacobi) and p.q <= 0 in
    pg_pcg_update_xr (forest); an iteration limit is reported as not done."""
    pg = _graph("chain119")
    h0 = _hook(ctx, "chain119", "jacobi", "lam0", 0)
    lam = -2 * np.abs(np.einsum("kii->ki", h0["H"][:h0["F"]])).max()
    hj = optimizer.debug_pg_solve(ctx, pg, lam, "jacobi", TOL, 64)
    assert hj["flags"][2] == 1
    hf = optimizer.debug_pg_solve(ctx, pg, lam, "forest", TOL, 64)
    assert hf["flags"][2] == 1 and hf["flags"][0] == 1
    for solver in ("forest", "jacobi"):
        h5 = optimizer.debug_pg_solve(ctx, pg, LAM0, solver, TOL, 5)
        assert h5["flags"][0] == 0 and h5["flags"][1] == 5 and h5["flags"][2] == 0
    big = _graph("chain2601")
    with pytest.raises(CcmError, match=r"error -1: .*forest does not fit"):        # CCM_E_ARG: F = 2601 > 2600
        optimizer.debug_pg_solve(ctx, big, LAM0, "forest", TOL, 0)
    assert optimizer.debug_pg_solve(ctx, big, LAM0, "jacobi", TOL, 0)["F"] == 2601   # the same graph is accepted by the solver that has no such limit


# ---- f. the product path --------------------------------------------------------------------------------------------------------------
# |chi2_final(pcg) - chi2_final(default)| / chi2_initial: 10 x the measured value, never above 1e-3
# measured: 1.80e-4 (120 keyframes: the PCG run takes 6 LM iterations / 6 trials where the exact solver takes 2 / 11), 4.32e-13 (120, fix_scale: both 5 / 5),
# 1.02e-4 (500: 16 / 16 against 2 / 11)
CHI2_BAR = {(120, False): 1.80e-3, (120, True): 4.32e-12, (500, False): 1.02e-3}


def _product(ctx, monkeypatch, pg, max_iters=20):
    monkeypatch.delenv("CCM_PG_SOLVER", raising=False)
    s0, st0 = optimizer.pose_graph_optimization(ctx, pg, max_iters)
    monkeypatch.setenv("CCM_PG_SOLVER", "pcg")
    s, st = optimizer.pose_graph_optimization(ctx, pg, max_iters)
    assert st0.pcg_iters == 0 and st.pcg_iters > 0
    fx = pg["fixed"] == 1
    assert np.array_equal(s[fx], pg["sim3"][fx])                          # fixed vertices untouched, bit for bit
    if pg["fix_scale"]:
        assert np.array_equal(s[:, 7], pg["sim3"][:, 7])                  # update[6] is zeroed: scales never move
    assert st.chi2_initial == st0.chi2_initial                            # the same kernels compute it
    assert st.chi2_final < 0.2 * st.chi2_initial
    d = abs(st.chi2_final - st0.chi2_final) / st.chi2_initial
    print("pcg iterations", st.pcg_iters, "LM", (st.iters_done, st.lm_trials), "default LM", (st0.iters_done, st0.lm_trials), "chi2 distance", d)
    return d


@pytest.mark.parametrize("n_kf,fix_scale", [(120, False), (120, True), (500, False)])
def test_product_path_with_the_forest_solver(ctx, monkeypatch, n_kf, fix_scale):
    """ccm_pose_graph_optimize with CCM_PG_SOLVER=pcg (forest PCG at these sizes) against the default exact solver"""
    pg = synth.make_pose_graph(n_kf, 1, fix_scale=fix_scale) if n_kf == 120 else synth.make_pose_graph(500, 2, covis=6)
    d = _product(ctx, monkeypatch, pg)
    assert d <= min(CHI2_BAR[(n_kf, fix_scale)], 1e-3)


def test_product_path_with_the_jacobi_solver(ctx, monkeypatch):
    """2602 keyframes: F = 2601 is past the forest's limit, so CCM_PG_SOLVER=pcg is block-Jacobi PCG; one LM iteration (measured: 29 840 CG
    iterations in its one trial, 0.7 s for both runs)"""
    _product(ctx, monkeypatch, _graph("chain2601"), max_iters=1)
