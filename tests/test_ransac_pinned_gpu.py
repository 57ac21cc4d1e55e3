"""GPU: the bits of ccm_sim3_ransac_eval and ccm_pnp_ransac_eval on one fixed small case against the digests recorded at the commit before the two kernels
were written over one wave skeleton (csrc/ransac_wave.h): tests/golden/ransac_pinned_digests.json holds that commit's id and the SHA-256 of n_inl, of the masks
and of the model output (rts, Rt) of both entry points.  The case: three candidates with N = S (3 for Sim3, 4 for PnP), 33 and 70 correspondences and 23
hypotheses interleaved over them.  Non-finite model values are replaced by one fixed NaN pattern before hashing (the sign of a default NaN is not portable)."""
import hashlib
import json
import os

import numpy as np
import pytest

import pnp_cases as pc
from ccm_slam_amd import pnp, sim3
from test_sim3_ransac_gpu import _cands

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ransac_pinned_digests.json")
H = 23


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _canonical(x):
    x = np.array(x, copy=True)
    f32 = x.dtype == np.float32
    x.view(np.uint32 if f32 else np.uint64)[~np.isfinite(x)] = 0x7fc00000 if f32 else 0x7ff8000000000000
    return x


def _digest(n_inl, model, masks):
    return dict(n_inl=_sha(np.asarray(n_inl, np.int32)), masks=_sha(np.concatenate([np.asarray(m, np.uint8) for m in masks])), model=_sha(_canonical(model)))


def sim3_case():
    cands = _cands(90, 3, 0, [3, 33, 70], 0.2)
    rng = np.random.default_rng(91)
    hc = (np.arange(H) % 3).astype(np.int32)
    hi = np.array([rng.choice(cands[c].N, 3, replace=False) for c in hc], np.int32)
    return cands, hc, hi


def pnp_case():
    cands = [pc.make_candidate(41, 4, 0, cam=(500.0, 510.0, 320.0, 240.0)), pc.make_candidate(42, 25, 8, cam=(420.5, 415.25, 300.0, 220.0)),
             pc.make_candidate(43, 50, 20, cam=(700.0, 690.0, 640.0, 360.0))]
    rng = np.random.default_rng(4)
    for k, c in enumerate(cands):
        c.sigma2 = ((1.2 ** rng.integers(0, 8, c.N)) ** 2).astype(np.float32) * np.float32(1 + k)
    hc = (np.arange(H) % 3).astype(np.int32)
    hi = np.array([rng.choice(cands[c].N, 4, replace=False) for c in hc], np.int32)
    return cands, hc, hi


def digests(ctx):
    """{entry point: {n_inl, masks, model}} of the fixed case on the device"""
    sc, shc, shi = sim3_case()
    pcands, phc, phi = pnp_case()
    return dict(ccm_sim3_ransac_eval=_digest(*sim3.eval_hypotheses(ctx, sc, shc, shi, False)), ccm_pnp_ransac_eval=_digest(*pnp.eval_hypotheses(ctx, pcands, phc, phi)))


def test_the_case_is_the_one_recorded():
    assert [c.N for c in sim3_case()[0]] == [3, 33, 70] and [c.N for c in pnp_case()[0]] == [4, 33, 70]
    want = json.load(open(GOLDEN))
    assert len(want["parent_commit"]) == 40 and set(want["digests"]) == {"ccm_sim3_ransac_eval", "ccm_pnp_ransac_eval"}


@pytest.mark.gpu
def test_device_bits_equal_those_recorded_before_the_skeleton(ctx):
    want = json.load(open(GOLDEN))["digests"]
    got = digests(ctx)
    n_sim3, _, m_sim3 = sim3.eval_hypotheses(ctx, *sim3_case(), False)
    assert n_sim3.max() > 6 and any(m.any() for m in m_sim3)   # the case has real inlier sets: the mask digest is not that of zeros
    assert got == want, (got, want)
