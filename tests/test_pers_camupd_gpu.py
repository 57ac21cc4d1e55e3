"""The camera update of an LM trial at the end of the persistent PCG launch (pers_update_cams) instead of a ba_update_cams launch behind it.  The per-camera
terms of the gain denominator go to cam_sc and ba_reduce_scalars re-forms the block sums ba_update_cams formed of them, so nothing a caller sees may move by a
bit: with CCM_BA_PERS_CAMUPD unset and =0 (the separate launch) the LM runs below must agree byte for byte with each other and with
tests/golden/pers_camupd_parent.npz, which scripts/record_pers_camupd_parent.py recorded with the library of the commit before the change (this project's own
outputs).  map70: 70 free cameras — a 6-camera last cluster whose second unit owns no camera, idle padded units; run(8) has a rejected trial, whose successor
loads the saved cluster inverse.  map179: 179 free cameras, a 3-camera last cluster."""
import contextlib
import hashlib
import os

import numpy as np
import pytest

from ccm_slam_amd import optimizer
from ccm_slam_amd._lib import K

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pers_camupd_parent.npz")
MAPS = ("map70", "map179")
ITERS = 8          # the first rejected trial of both maps comes at LM iteration 7
SETTINGS = (None, "0")
_TPB, _WAVE = 256, 64   # ba_update_cams' workgroup (kTPB) and the wave


def problem(name):
    from tests.test_pcg_wave0_path_gpu import problem as p
    return p(name)


@contextlib.contextmanager
def _camupd(setting):
    """CCM_BA_PERS_CAMUPD as the handle's creation will read it: None = unset (on), "0" = the separate ba_update_cams launch."""
    old = os.environ.pop("CCM_BA_PERS_CAMUPD", None)
    if setting is not None:
        os.environ["CCM_BA_PERS_CAMUPD"] = setting
    try:
        yield
    finally:
        os.environ.pop("CCM_BA_PERS_CAMUPD", None)
        if old is not None:
            os.environ["CCM_BA_PERS_CAMUPD"] = old


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def lm_run(ctx, name, setting, read_flags=True):
    """run(ITERS) of the map on a handle created under the setting.  Returns what a caller can see — counts, history(), the downloaded cameras, points, chi2
    per edge and depth flags — plus the launches of three kernel classes and (read_flags) the last trial's PCG flags and the persistent kernel's abort words."""
    with _camupd(setting):
        h = optimizer.BAHandle(ctx, problem(name))
    try:
        ctx.prof_enable(-1); ctx.prof_reset()
        st = h.run(ITERS)
        launches = {k: ctx.prof_read(K[k])[0] for k in ("BA_UPDATE", "BA_PCG_PERSIST", "BA_PCG_SPMV")}
        ctx.prof_enable(-2)
        chi, lam, trials = h.history()
        cam, pts, chi2, dpos = h.download()
        out = dict(counts=np.array([st.iters_done, st.lm_trials, st.pcg_iters], np.int32), free_cams=h.counts()["free_cams"], pers_grid=h.debug_sizes()["pers_grid"],
                   hist_chi2=chi, hist_lambda=lam, hist_trials=trials, cam=cam, pts=pts, chi2=chi2, dpos=dpos, launches=launches)
        if read_flags:
            from tests.test_ba_structure_gpu import dev_array
            out["pcg_flag"] = dev_array(h, "pcg_flag", np.int32)
            out["pers_flags"] = dev_array(h, "pers_flags", np.uint32)
        return out
    finally:
        h.close()


def fixture_record(res):
    """What the fixture keeps of one run: the small arrays as they are, the large ones by their sha256."""
    return dict(counts=res["counts"], hist_chi2=res["hist_chi2"], hist_lambda=res["hist_lambda"], hist_trials=res["hist_trials"], cam=res["cam"],
                pts_sha256=np.array(_sha(res["pts"])), chi2_sha256=np.array(_sha(res["chi2"])), dpos_sha256=np.array(_sha(res["dpos"])))


_runs = {}


def _run(ctx, name, setting):
    """every (map, setting) runs once for all the tests of this file; nobody changes the result"""
    if (name, setting) not in _runs:
        _runs[(name, setting)] = lm_run(ctx, name, setting)
    return _runs[(name, setting)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", MAPS)
def test_both_settings_give_the_same_bytes(ctx, name):
    on, off = _run(ctx, name, None), _run(ctx, name, "0")
    assert on["free_cams"] == {"map70": 70, "map179": 179}[name]
    if name == "map70":   # 10 units in a grid of 16: idle padded units
        assert on["pers_grid"] > 2 * ((on["free_cams"] + 15) // 16)
        assert on["counts"][1] > on["counts"][0]   # a rejected trial
    for key in ("counts", "hist_chi2", "hist_lambda", "hist_trials", "cam", "pts", "chi2", "dpos"):
        assert on[key].tobytes() == off[key].tobytes(), key


@pytest.mark.gpu
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", MAPS)
def test_reproduces_the_parent(ctx, name, setting):
    g = np.load(GOLDEN)
    rec = fixture_record(_run(ctx, name, setting))
    assert set(k for k in g.files if k.startswith(name + "_")) == set(name + "_" + k for k in rec)
    for key, val in rec.items():
        exp = g[name + "_" + key]
        if key.endswith("_sha256"):
            assert str(val) == str(exp), key
        else:
            assert val.dtype == exp.dtype and val.shape == exp.shape and val.tobytes() == exp.tobytes(), key


@pytest.mark.gpu
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", MAPS)
def test_launches_and_flags(ctx, name, setting):
    """Every trial is one persistent launch that ends clean; the separate camera-update launch is gone with the switch unset and is there once per trial with =0;
    the abort words are clear for the next launch."""
    res = _run(ctx, name, setting)
    trials = int(res["counts"][1])
    assert res["launches"]["BA_PCG_PERSIST"] == trials and res["launches"]["BA_PCG_SPMV"] == 0, res["launches"]
    assert res["launches"]["BA_UPDATE"] == (0 if setting is None else trials), res["launches"]
    assert res["pcg_flag"][2] == 0 and res["pcg_flag"][3] == 0, res["pcg_flag"]
    assert not res["pers_flags"].any(), res["pers_flags"]


# ---- the order of the sums, on the CPU ----

def _wave_sum(v):
    """lanex::wave_sum: the xor butterfly 32, 16, 8, 4, 2, 1 over 64 lanes; every lane ends with the same bits (a + b and b + a are the same double)"""
    v = np.array(v, np.float64)
    lanes = np.arange(_WAVE)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ off]
    assert (v == v[0]).all() or np.isnan(v).all()
    return v[0]


def _block_sum(v):
    """block_sum of ba.hip over the 256 threads of a workgroup: the wave sums, then thread 0 adds them in wave order starting from 0"""
    s = np.float64(0.0)
    for w in range(_TPB // _WAVE):
        s = s + _wave_sum(v[_WAVE * w:_WAVE * (w + 1)])
    return s


def update_cams_scale(terms, part_pt_sc):
    """The parent: workgroup b of ba_update_cams block-sums the terms of cameras [256 b, 256 b + 256) (threads beyond Cp hold 0) into part_cam[b]; thread i of
    ba_reduce_scalars adds part_cam[i] to its thread-strided sum of the landmark-side partials; block_sum of the 256 threads."""
    cp = terms.size
    n_wg = (cp + _TPB - 1) // _TPB
    part_cam = np.zeros(n_wg)
    for b in range(n_wg):
        v = np.zeros(_TPB)
        v[:min(_TPB, cp - _TPB * b)] = terms[_TPB * b:_TPB * (b + 1)]
        part_cam[b] = _block_sum(v)
    sc = np.zeros(_TPB)
    for t in range(_TPB):
        for i in range(t, part_pt_sc.size, _TPB):
            sc[t] = sc[t] + part_pt_sc[i]
        for i in range(t, n_wg, _TPB):
            sc[t] = sc[t] + part_cam[i]
    return _block_sum(sc), part_cam


def restated_scale(cam_sc, part_pt_sc, batch=8, max_blocks=16):
    """The change: thread t of ba_reduce_scalars holds cs[q] = cam_sc[256 q + t] for every block q at once (0 beyond Cp), takes the wave butterfly of each, the
    first lane of every wave parks the wave sums, and thread b adds block b's four in wave order starting from 0, then adds that to its sum of the landmark-side
    partials — which it has requested `batch` at a time and added in index order."""
    cp = cam_sc.size
    n_wg = (cp + _TPB - 1) // _TPB
    assert n_wg <= max_blocks
    cs = np.zeros((max_blocks, _TPB))
    for q in range(n_wg):
        for t in range(_TPB):
            if _TPB * q + t < cp:
                cs[q, t] = cam_sc[_TPB * q + t]
    cam_ws = np.zeros((max_blocks, _TPB // _WAVE))
    for q in range(n_wg):
        for w in range(_TPB // _WAVE):
            cam_ws[q, w] = _wave_sum(cs[q, _WAVE * w:_WAVE * (w + 1)])
    sc = np.zeros(_TPB)
    for t in range(_TPB):
        for i0 in range(t, part_pt_sc.size, batch * _TPB):
            v = [part_pt_sc[i0 + q * _TPB] if i0 + q * _TPB < part_pt_sc.size else 0.0 for q in range(batch)]
            for q in range(batch):
                if i0 + q * _TPB < part_pt_sc.size:
                    sc[t] = sc[t] + v[q]
    part = np.zeros(n_wg)
    for b in range(n_wg):
        s = np.float64(0.0)
        for w in range(_TPB // _WAVE):
            s = s + cam_ws[b, w]
        part[b] = s
        sc[b] = sc[b] + s
    return _block_sum(sc), part


@pytest.mark.parametrize("cp", [70, 179, 256, 257, 2000])
def test_restated_block_sums_keep_the_order(cp):
    """Terms of mixed sign over twelve decades, where a regrouped sum differs in its last bits: the block sums and `scale` of the two formulations are the same
    doubles."""
    rng = np.random.default_rng(cp)
    terms = rng.standard_normal(cp) * 10.0 ** rng.uniform(-6, 6, cp)
    part_pt_sc = rng.standard_normal(3730) * 10.0 ** rng.uniform(-6, 6, 3730)
    a, part_a = update_cams_scale(terms, part_pt_sc)
    b, part_b = restated_scale(terms, part_pt_sc)
    assert part_a.tobytes() == part_b.tobytes()
    assert np.float64(a).tobytes() == np.float64(b).tobytes()
