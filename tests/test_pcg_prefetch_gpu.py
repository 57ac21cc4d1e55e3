"""The persistent PCG's partner w and coarse parts travel tagged ({bits, bits ^ key(epoch)}) and are fetched by waves 1..15 INSIDE the
grid-wide exchange (CCM_BA_PERS_PREFETCH, default on; 0 = right after it, the schedule before the change).  This is a scheduling change: every
sum keeps its operands and order, so both settings, and the library before the change (tests/golden/pcg_prefetch_parent.npz), must agree
byte for byte.  A launch that gave up waiting (pcg_flag[3]) or failed numerically (pcg_flag[2]) fails the test."""
import contextlib
import os

import numpy as np
import pytest

from ccm_slam_amd import optimizer, synth
from ccm_slam_amd._lib import K
from tests.test_pcg_one_exchange_gpu import _pers_solve, _problem, _reduced

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pcg_prefetch_parent.npz")
CASES = [(coarse, scale) for coarse in (True, False) for scale in (1e-5, 1e-1)]   # lambda = scale x the largest diagonal entry of S


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


def _solves(ctx, prob, setting, lams=None):
    """One handle created under the setting; the four solves of CASES.  Returns ({case: (x, flags)}, {scale: lambda}, counts, sizes)."""
    with _prefetch(setting):
        h = optimizer.BAHandle(ctx, prob)
    try:
        if lams is None:
            B0, bi, bj, _ = _reduced(h, 1.0)
            dmax = max(np.diagonal(B0[k]).max() for k in np.flatnonzero(bi == bj))
            lams = {scale: scale * dmax for _, scale in CASES}
        assert h.coarse_level(1.0)[0] > 0
        out = {}
        for coarse, scale in CASES:
            x, fl = _pers_solve(h, lams[scale], coarse)
            out[(coarse, scale)] = (x, fl.copy())
        return out, lams, h.counts(), h.debug_sizes()
    finally:
        h.close()


def _assert_same(on, off):
    for case in CASES:
        (x1, f1), (x0, f0) = on[case], off[case]
        assert f1[2] == 0 and f1[3] == 0 and f0[2] == 0 and f0[3] == 0, (case, f1, f0)
        assert f1[1] > 0 and f1[1] == f0[1], (case, f1, f0)
        assert x1.tobytes() == x0.tobytes(), (case, np.abs(x1 - x0).max())


@pytest.fixture(scope="module")
def map179(ctx):
    prob = _problem("map179")
    on, lams, counts, _ = _solves(ctx, prob, None)
    off, _, _, _ = _solves(ctx, prob, "0")
    return dict(prob=prob, on=on, off=off, lams=lams, counts=counts)


@pytest.mark.gpu
def test_prefetch_on_and_off_give_the_same_bits(map179):
    """map179: 179 free cameras, so the last cluster's second unit owns no row.  Coarse level on and off, lambda 1e-5 and 1e-1 of the largest
    diagonal entry: x equal as bytes, the same iteration count, no give-up and no numeric failure."""
    assert map179["counts"]["free_cams"] == 179
    _assert_same(map179["on"], map179["off"])


@pytest.mark.gpu
def test_idle_padded_workgroups_and_an_odd_tail(ctx):
    """A one-agent map whose last cluster is at most half full (its second unit owns no row, the first an odd number) and whose unit count is no
    multiple of 8, so the grid is padded with workgroups that own nothing but still take part in every exchange and fetch the coarse parts."""
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=78, n_points=4000, n_fixed=8, fixed_mode="tail", seed=2070)
    on, lams, counts, sizes = _solves(ctx, prob, None)
    cp = counts["free_cams"]
    units = 2 * ((cp + 15) // 16)
    assert 51 <= cp <= 120 and 1 <= cp % 16 <= 8, cp
    assert units % 8 != 0 and sizes["pers_grid"] > units, (units, sizes["pers_grid"])
    off, _, _, _ = _solves(ctx, prob, "0", lams)
    _assert_same(on, off)


@pytest.mark.gpu
@pytest.mark.parametrize("setting", [None, "0"])
def test_both_settings_reproduce_the_parent_commit(ctx, map179, setting):
    """x and the iteration counts of the four map179 solves as a library built from the commit before this change gave them (the golden file holds
    this project's own outputs, and the lambdas they were taken at): both places of the fetch reproduce them byte for byte."""
    g = np.load(GOLDEN)
    lams = {scale: float(g["lam"][i]) for i, scale in enumerate((1e-5, 1e-1))}
    assert lams == map179["lams"]   # the reduced system itself has not moved
    got = map179["on"] if setting is None else map179["off"]
    for i, case in enumerate(CASES):
        x, fl = got[case]
        assert (bool(g["coarse"][i]), float(g["scale"][i])) == case
        assert int(fl[1]) == int(g["iters"][i]) and fl[2] == 0 and fl[3] == 0, (case, fl, int(g["iters"][i]))
        assert x.tobytes() == g["x"][i].tobytes(), (case, np.abs(x - g["x"][i]).max())


@pytest.mark.gpu
def test_lm_run_is_the_same_with_the_fetch_inside_or_after_the_exchange(ctx):
    """gba_c3, run(10): the same LM iterations, trials and CG iterations, cameras and points equal as bytes, and no trial fell back to the
    multi-kernel solver (no BA_PCG_SPMV launch)."""
    prob = synth.make_ba_config("gba_c3")
    res = []
    for setting in (None, "0"):
        with _prefetch(setting):
            h = optimizer.BAHandle(ctx, prob)
        ctx.prof_enable(-1); ctx.prof_reset()
        st = h.run(10)
        n_pers, _ = ctx.prof_read(K["BA_PCG_PERSIST"])
        n_spmv, _ = ctx.prof_read(K["BA_PCG_SPMV"])
        ctx.prof_enable(-2)
        cam, pts, _, _ = h.download()
        h.close()
        assert n_pers > 0 and n_spmv == 0, (setting, n_pers, n_spmv)
        res.append((st, cam, pts))
    (s1, c1, p1), (s0, c0, p0) = res
    assert (s1.iters_done, s1.lm_trials, s1.pcg_iters) == (s0.iters_done, s0.lm_trials, s0.pcg_iters)
    assert c1.tobytes() == c0.tobytes() and p1.tobytes() == p0.tobytes()
