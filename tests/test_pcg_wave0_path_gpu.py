"""The persistent PCG with a cheaper grid exchange: the slots and u move as 16-byte records, and the units' parts of P^T b are published before
the factorisation and gathered without a grid exchange.  (Moving the coarse restriction from wave 0 to wave 15 was measured against the same
tests and dropped: DESIGN 4.1.)  These are scheduling / transport changes: every sum keeps its operands and order, so the solver must reproduce
the library of the commit before the change byte for byte, with CCM_BA_PERS_PREFETCH unset and =0.  tests/golden/pcg_prefetch_parent.npz (map179, recorded two changes
ago, only read here) and tests/golden/pcg_wave0_parent.npz (scripts/record_pcg_wave0_parent.py, run with the parent's library) hold this
project's own outputs.  A launch that gave up waiting (pcg_flag[3]) or failed numerically (pcg_flag[2]) fails the test."""
import contextlib
import hashlib
import os

import numpy as np
import pytest

from ccm_slam_amd import optimizer, synth
from ccm_slam_amd._lib import K
from tests.test_pcg_one_exchange_gpu import _pers_solve, _problem, _reduced

_GOLDEN_DIR = os.path.join(os.path.dirname(__file__), "golden")
GOLDEN_MAP179 = os.path.join(_GOLDEN_DIR, "pcg_prefetch_parent.npz")
GOLDEN = os.path.join(_GOLDEN_DIR, "pcg_wave0_parent.npz")
CASES = [(coarse, scale) for coarse in (True, False) for scale in (1e-5, 1e-1)]   # lambda = scale x the largest diagonal entry of S
SCALES = (1e-5, 1e-1)
# The LM run in which a rejected trial's successor loads the saved cluster inverse W with the coarse level on (P^T b is then published only ~5 us
# before it is gathered).  run(3) of map179 has no rejected trial, and neither has run(3) of any synth map on the persistent solver's path: lambda
# falls by 3 with every accepted step, and the first rejection comes at LM iteration 7 (map70, lba62, map179) or 8 (gba_c3), on the CPU oracle and on
# the device alike.  So the run is run(8) of the smallest such map.  The recording script takes the first candidate that has such a trial with the
# parent's library, and the fixture names it.
LM_CANDIDATES = (("map179", 3), ("map70", 8), ("lba62", 8), ("map179", 8))
LM_CASE = ("map70", 8)


def problem(name):
    if name == "map70":   # one agent, 70 free cameras: 10 units, so the grid of 16 has idle padded units
        return synth.make_ba_problem(n_agents=1, kfs_per_agent=78, n_points=4000, n_fixed=8, fixed_mode="tail", seed=2070)
    if name == "lba62":
        return synth.make_ba_problem(n_agents=1, kfs_per_agent=70, n_points=4000, n_fixed=8, fixed_mode="tail", seed=2062)
    return _problem(name)


@contextlib.contextmanager
def _prefetch(setting):
    """CCM_BA_PERS_PREFETCH as the handle's creation will read it: None = unset (on), "0" = off."""
    old = os.environ.pop("CCM_BA_PERS_PREFETCH", None)
    if setting is not None:
        os.environ["CCM_BA_PERS_PREFETCH"] = setting
    try:
        yield
    finally:
        os.environ.pop("CCM_BA_PERS_PREFETCH", None)
        if old is not None:
            os.environ["CCM_BA_PERS_PREFETCH"] = old


def solves(ctx, prob, setting):
    """One handle created under the setting; the four solves of CASES.  Returns ({case: (x, flags)}, {scale: lambda}, counts, sizes)."""
    with _prefetch(setting):
        h = optimizer.BAHandle(ctx, prob)
    try:
        B0, bi, bj, _ = _reduced(h, 1.0)
        dmax = max(np.diagonal(B0[k]).max() for k in np.flatnonzero(bi == bj))
        lams = {scale: scale * dmax for scale in SCALES}
        assert h.coarse_level(1.0)[0] > 0
        out = {}
        for coarse, scale in CASES:
            x, fl = _pers_solve(h, lams[scale], coarse)
            out[(coarse, scale)] = (x, fl.copy())
        return out, lams, h.counts(), h.debug_sizes()
    finally:
        h.close()


def lm_run(ctx, prob, iters, setting=None):
    """An ordinary LM run.  Returns ((LM iterations, trials, CG iterations), sha256 of the cameras, of the points, persistent launches, BA_PCG_SPMV launches)."""
    with _prefetch(setting):
        h = optimizer.BAHandle(ctx, prob)
    try:
        ctx.prof_enable(-1); ctx.prof_reset()
        st = h.run(iters)
        n_pers, _ = ctx.prof_read(K["BA_PCG_PERSIST"])
        n_spmv, _ = ctx.prof_read(K["BA_PCG_SPMV"])
        ctx.prof_enable(-2)
        cam, pts, _, _ = h.download()
    finally:
        h.close()
    counts = (int(st.iters_done), int(st.lm_trials), int(st.pcg_iters))
    return counts, hashlib.sha256(cam.tobytes()).hexdigest(), hashlib.sha256(pts.tobytes()).hexdigest(), n_pers, n_spmv


def _assert_solves_equal(got, g, prefix, lams):
    assert {s: float(g[prefix + "lam"][i]) for i, s in enumerate(SCALES)} == lams   # the reduced system itself has not moved
    for i, case in enumerate(CASES):
        x, fl = got[case]
        assert (bool(g[prefix + "coarse"][i]), float(g[prefix + "scale"][i])) == case
        assert fl[2] == 0 and fl[3] == 0, (case, fl)
        assert int(fl[1]) > 0 and int(fl[1]) == int(g[prefix + "iters"][i]), (case, fl, int(g[prefix + "iters"][i]))
        assert x.tobytes() == g[prefix + "x"][i].tobytes(), (case, np.abs(x - g[prefix + "x"][i]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("setting", [None, "0"])
def test_map179_reproduces_the_recording_of_two_changes_ago(ctx, setting):
    """map179: 179 free cameras, the last cluster's second unit owns no row (it still publishes zero parts of P^T b and P^T w, which the interval's
    readers wait for).  Coarse level on and off, lambda 1e-5 and 1e-1 of the largest diagonal entry: x and the iteration counts equal the fixture byte for byte."""
    got, lams, counts, _ = solves(ctx, _problem("map179"), setting)
    assert counts["free_cams"] == 179
    _assert_solves_equal(got, np.load(GOLDEN_MAP179), "", lams)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", [None, "0"])
def test_padded_grid_reproduces_the_parent(ctx, setting):
    """The 70-camera map: its unit count is no multiple of 8, so the grid has idle padded units, which restrict nothing and whose parts have no
    reader, but whose 32-byte slots every unit polls.  The same four solves against the parent's recording."""
    got, lams, counts, sizes = solves(ctx, problem("map70"), setting)
    cp = counts["free_cams"]
    units = 2 * ((cp + 15) // 16)
    assert units % 8 != 0 and sizes["pers_grid"] > units, (cp, units, sizes["pers_grid"])
    _assert_solves_equal(got, np.load(GOLDEN), "map70_", lams)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", [None, "0"])
def test_lm_run_with_loaded_inverse_reproduces_the_parent(ctx, setting):
    """A short LM run through the ordinary loop: the coarse level is on and at least one rejected trial loads W (the fixture counts them on the
    parent), so P^T b is published just before it is gathered.  Counts and the digests of cameras and points as the parent gave them; no fall-back."""
    g = np.load(GOLDEN)
    assert (str(g["lm_case"]), int(g["lm_iters"])) == LM_CASE and int(g["lm_w_loads"]) > 0
    counts, cam_sha, pts_sha, n_pers, n_spmv = lm_run(ctx, problem(LM_CASE[0]), LM_CASE[1], setting)
    assert n_pers > 0 and n_spmv == 0, (n_pers, n_spmv)
    assert counts == tuple(int(v) for v in g["lm_counts"]), (counts, g["lm_counts"])
    assert counts[1] > counts[0]   # a rejected trial
    assert (cam_sha, pts_sha) == (str(g["lm_cam_sha256"]), str(g["lm_pts_sha256"]))


@pytest.mark.gpu
def test_gba_c3_run_reproduces_the_parent(ctx):
    """gba_c3, run(10): LM iterations, trials, CG iterations and the digests of cameras and points as the parent gave them; no fall-back."""
    g = np.load(GOLDEN)
    counts, cam_sha, pts_sha, n_pers, n_spmv = lm_run(ctx, problem("gba_c3"), 10)
    assert n_pers > 0 and n_spmv == 0, (n_pers, n_spmv)
    assert counts == tuple(int(v) for v in g["c3_counts"]), (counts, g["c3_counts"])
    assert (cam_sha, pts_sha) == (str(g["c3_cam_sha256"]), str(g["c3_pts_sha256"]))
