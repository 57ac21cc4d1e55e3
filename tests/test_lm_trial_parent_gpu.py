"""A pin of the LM trial driver (lm_trial of ba.hip) on every reduced solver it can pick: the register Cholesky, the exact two-cluster solve, the
single-workgroup PCG (first lambda given, and from ba_maxdiag), the persistent PCG and the multi-kernel PCG (coarse level by the switch, and always on).
A change of the HOST driver alone leaves the device code and the order of the stream's commands as they were, so every run below must hand its caller the
bytes of tests/golden/lm_trial_parent.npz, which scripts/record_lm_trial_parent.py recorded with the library of the commit before such a change (this
project's own outputs), and must count the same launches in every CCM_K_BA_* class.  The other parent pins of this suite reach the persistent path only.

map70: 70 free cameras; ITERS_MAP70 = 8 has a rejected trial on the persistent path (its successor loads the saved cluster inverse) and on the
multi-kernel path alike (asserted below, so the repeat at another lambda on the same linearisation is really in the pin)."""
import contextlib
import hashlib
import os

import numpy as np
import pytest

from ccm_slam_amd import optimizer, synth
from ccm_slam_amd._lib import K

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "lm_trial_parent.npz")
BA_CLASSES = tuple(k for k in K if k.startswith("BA_"))   # in the enum's order
ENV_NAMES = ("CCM_BA_CHOLREG", "CCM_BA_NO_PERSIST", "CCM_BA_COARSE")   # read when the handle is created
ITERS_SMALL, ITERS_MAP70 = 5, 8
LAMBDA_GIVEN = 1.0
# name: (problem, env at creation, LM iterations, lambda_init, solver)
CASES = {
    "cholreg18": (("synth", 19, 60 * 19, 119), {}, ITERS_SMALL, 0.0, "cholreg"),
    "dense2_20": (("synth", 21, 60 * 21, 221), {"CCM_BA_CHOLREG": "0"}, ITERS_SMALL, 0.0, "dense2"),
    "small11_lambda_given": (("synth", 12, 700, 500), {}, ITERS_SMALL, LAMBDA_GIVEN, "pcg_small"),
    "small11_maxdiag": (("synth", 12, 700, 500), {}, ITERS_SMALL, 0.0, "pcg_small"),
    "map70_persist": (("map70",), {}, ITERS_MAP70, 0.0, "pcg_persist"),
    "map70_multi_kernel": (("map70",), {"CCM_BA_NO_PERSIST": "1"}, ITERS_MAP70, 0.0, "multi_kernel"),
    "map70_mk_coarse_always": (("map70",), {"CCM_BA_NO_PERSIST": "1", "CCM_BA_COARSE": "always"}, ITERS_MAP70, 0.0, "multi_kernel"),
}
BYTE_KEYS = ("cam", "pts_sha256", "chi2_sha256", "dpos_sha256")   # left out of a case whose two recordings on the parent differed
ALWAYS_KEYS = ("counts", "hist_chi2", "hist_lambda", "hist_trials", "launches")


def problem(spec):
    if spec[0] == "map70":
        from tests.test_pcg_wave0_path_gpu import problem as p
        return p("map70")
    _, kfs, n_points, seed = spec
    return synth.make_ba_problem(n_agents=1, kfs_per_agent=kfs, n_points=n_points, seed=seed)


@contextlib.contextmanager
def _env(settings):
    """the switches a handle's creation reads: the named ones set, the others unset"""
    old = {k: os.environ.pop(k, None) for k in ENV_NAMES}
    os.environ.update(settings)
    try:
        yield
    finally:
        for k in ENV_NAMES:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def lm_run(ctx, name):
    """One LM run of the case.  Returns what the fixture keeps of it (the small arrays as they are, the large ones by their sha256, the launches of every
    BA class) plus `sizes`."""
    spec, env, iters, lam0, _ = CASES[name]
    with _env(env):
        h = optimizer.BAHandle(ctx, problem(spec))
    try:
        sz = h.debug_sizes()
        ctx.prof_enable(-1); ctx.prof_reset()
        st = h.run(iters, lambda_init=lam0)
        launches = np.array([ctx.prof_read(K[k])[0] for k in BA_CLASSES], np.int64)
        ctx.prof_enable(-2)
        chi, lam, trials = h.history()
        cam, pts, chi2, dpos = h.download()
    finally:
        h.close()
    return dict(counts=np.array([st.iters_done, st.lm_trials, st.pcg_iters], np.int32), hist_chi2=chi, hist_lambda=lam, hist_trials=trials, launches=launches,
                cam=cam, pts_sha256=np.array(_sha(pts)), chi2_sha256=np.array(_sha(chi2)), dpos_sha256=np.array(_sha(dpos)), sizes=sz)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and (str(a) == str(b) if a.dtype.kind == "U" else a.tobytes() == b.tobytes())


_runs = {}


def _run(ctx, name):
    """every case runs once for all the tests of this file; nobody changes the result"""
    if name not in _runs:
        _runs[name] = lm_run(ctx, name)
    return _runs[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_reproduces_the_parent(ctx, name):
    g = np.load(GOLDEN)
    assert tuple(str(k) for k in g["ba_classes"]) == BA_CLASSES
    res = _run(ctx, name)
    keys = ALWAYS_KEYS + (BYTE_KEYS if bool(g[name + "_reproducible"]) else ())
    assert set(k for k in g.files if k.startswith(name + "_")) == set(name + "_" + k for k in keys + ("reproducible",))
    got, exp = dict(zip(BA_CLASSES, res["launches"].tolist())), dict(zip(BA_CLASSES, g[name + "_launches"].tolist()))
    assert got == exp, {k: (got[k], exp[k]) for k in BA_CLASSES if got[k] != exp[k]}
    for key in keys:
        assert same(res[key], g[name + "_" + key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_the_case_reaches_its_solver(ctx, name):
    """which reduced solver ran, as tests/test_ba_one_trial_gpu.py tells them apart; the map70 runs have a rejected trial"""
    res = _run(ctx, name)
    solver, sz, n = CASES[name][4], res["sizes"], dict(zip(BA_CLASSES, res["launches"].tolist()))
    trials, pcg_iters = int(res["counts"][1]), int(res["counts"][2])
    if solver == "cholreg":
        ok = n["BA_PCG_PERSIST"] == trials and n["BA_PCG_SPMV"] == 0 and sz["pers_grid"] == 0 and 16 < sz["Cp"] <= 50 and pcg_iters == trials
    elif solver == "dense2":
        ok = n["BA_PCG_PERSIST"] == trials and n["BA_PCG_SPMV"] == 0 and sz["pers_grid"] > 0 and 16 < sz["Cp"] <= 32 and pcg_iters == trials
    elif solver == "pcg_small":
        ok = n["BA_PCG_PERSIST"] == 0 and n["BA_PCG_SPMV"] == trials and sz["Cp"] <= 16 and pcg_iters > trials
    elif solver == "pcg_persist":
        ok = n["BA_PCG_PERSIST"] == trials and n["BA_PCG_SPMV"] == 0 and sz["pers_grid"] > 0 and sz["Cp"] > 50 and pcg_iters > trials
    else:
        ok = n["BA_PCG_PERSIST"] == 0 and n["BA_PCG_SPMV"] > trials and sz["pers_grid"] == 0 and sz["Cp"] > 50 and pcg_iters > trials
    assert ok, (name, solver, n, sz, res["counts"])
    if name == "map70_mk_coarse_always":
        assert n["BA_COARSE"] > 0
    if CASES[name][0] == ("map70",):
        assert sz["Cp"] == 70 and trials > int(res["counts"][0]), res["counts"]   # a rejected trial
