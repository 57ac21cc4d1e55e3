"""SearchAndFuse on the CPU: csrc/fuse_math.h compiled by g++ (libccm_host.so) against the reference's own ORBmatcher::Fuse(pKF, Scw, ...)
(oracle/_ref/libmatcher_ref.so through ref_fuse_sim3, kf_has_mp all zero, one call per keyframe), against oracle.grid_candidates plus a numpy arg-min for the three
outcomes the reference does not tell apart, and against hand-made pairs with known answers; the mirror cslam::SearchAndFuseBatch with the host evaluator through a
walk of eight Fuse calls between which the map changes; every CCM_E_ARG case.  Every comparison is exact: integers, and float bit patterns for u and v."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import tests.test_ref_matcher as trm
from ccm_slam_amd import fuse_sim3 as fs, synth
from ccm_slam_amd._lib import CcmError
from fuse_sim3_cases import (TH, assert_reference_scene, disc, DISC_SIZES, planted, ref_fuse, same_as_reference, scene_from_frames)

KINDS = "nnffnnff"
needs_ref = pytest.mark.skipif(not os.path.exists(trm.LIB) and not os.path.isdir("/root/reference/cslam"), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def frames():
    o = oracle.OrbOracle(1000)
    out = [o.extract(synth.gen_image(1000, t)) for t in (0, 1)]
    o.close()
    return out


@pytest.fixture(scope="module")
def mixed(frames):
    """the 8-keyframe scene (4 near, 4 far) and the host evaluator's answer, computed once"""
    sc, s, S16, which = scene_from_frames(frames, KINDS)
    return sc, s, S16, which, fs.fuse_sim3_eval_host(sc, want_uv=True, want_cand=True)


@pytest.fixture(scope="module")
def refs(frames, mixed):
    if not os.path.exists(trm.LIB):
        from oracle import ref
        ref.build()
    rlib = C.CDLL(trm.LIB)
    sc, s, S16, which, _ = mixed
    out = [ref_fuse(rlib, frames, s, S16, which, k) for k in range(len(KINDS))]
    assert_reference_scene(out, KINDS)
    return rlib, out


def test_build_grid_is_the_oracles_grid(frames):
    for kps, _ in frames:
        off, idx = fs.build_grid(np.stack([kps["x"], kps["y"]], 1), trm.BOUNDS)
        eoff, eidx = oracle.build_grid(kps["x"], kps["y"], trm.BOUNDS)
        assert np.array_equal(off, eoff) and np.array_equal(idx, eidx)
    with pytest.raises(ValueError):
        fs.build_grid([[751.0, 10.0]], trm.BOUNDS)


@needs_ref
def test_host_evaluator_equals_the_references_fuse_for_every_keyframe(mixed, refs):
    sc, s, S16, which, got = mixed
    t = fs.unpack_table(got["table"])
    for k in range(sc.K):
        same_as_reference({n: a[k] for n, a in t.items()}, got["uv"][k], refs[1][k], f"keyframe {k}")
        assert got["n_valid"][k] == refs[1][k][2].sum() and got["n_hit"][k] == refs[1][k][0]


def test_statuses_4_5_6_against_the_oracles_grid_and_a_numpy_arg_min(frames, mixed):
    """what the reference reports as 'not fused' in three flavours: window empty, nobody at the level, best distance above TH_LOW"""
    sc, s, S16, which, got = mixed
    t = fs.unpack_table(got["table"])
    seen = set()
    for k in range(sc.K):
        kps, desc = frames[which[k]]
        m = np.flatnonzero(t["status"][k] >= 4)
        u, v, lvl = got["uv"][k, m, 0], got["uv"][k, m, 1], t["level"][k, m]
        r = (np.float32(TH) * s["sf"][lvl]).astype(np.float32)
        none = -np.ones(m.size, np.int32)
        aoff, _ = oracle.grid_candidates(kps["x"], kps["y"], kps["octave"], trm.BOUNDS, u, v, r, none, none)
        loff, lidx = oracle.grid_candidates(kps["x"], kps["y"], kps["octave"], trm.BOUNDS, u, v, r, (lvl - 1).astype(np.int32), lvl.astype(np.int32))
        assert np.array_equal(np.diff(aoff), got["n_cand"][k, m]), k
        bits = np.unpackbits(desc, axis=1).astype(np.int16); qbits = np.unpackbits(s["pdesc"][m], axis=1).astype(np.int16)
        for j, i in enumerate(m):
            st = int(t["status"][k, i])
            if aoff[j + 1] == aoff[j]:
                exp = (4, -1, -1)
            elif loff[j + 1] == loff[j]:
                exp = (5, -1, -1)
            else:
                cand = lidx[loff[j]:loff[j + 1]]
                d = np.abs(bits[cand] - qbits[j]).sum(1)
                b = int(np.argmin(d))                   # the first minimum, in the reference's candidate order
                exp = (7 if d[b] <= 50 else 6, int(cand[b]), int(d[b]))
            assert (st, int(t["idx"][k, i]), int(t["dist"][k, i])) == exp, (k, i)
            seen.add(st)
    assert seen == {4, 5, 6, 7}


def test_planted_boundaries_have_their_known_answers():
    pl = planted()
    got = fs.fuse_sim3_eval_host(pl.scene(), want_uv=True)
    pl.check(got["table"], "host")
    t = fs.unpack_table(got["table"])
    assert np.array_equal(got["n_valid"], (t["status"] >= 4).sum(1)) and np.array_equal(got["n_hit"], (t["status"] == 7).sum(1))
    # the exact projections behind the bounds cases: points 3 .. 10 of keyframe 0
    assert got["uv"][0, 3:11].tolist() == [[0, 224], [752, 224], [304, 0], [304, 480], [-2.0 ** -15, 224], [744, 224], [304, -2.0 ** -16], [304, 472]]


def test_decompose_scw_follows_the_matrix_rules():
    """Mat::dot in double, scw a float, Mat / s = Mat * (float)(1. / s) in float, -Rcw.t() * tcw one double-accumulated gemm: restated with numpy scalars"""
    rng = np.random.default_rng(3)
    for _ in range(50):
        S = fs.perturbed_scw(rng, float(rng.uniform(0.3, 3)), 0.5, 1.0)
        A = S.reshape(3, 4)
        scw = np.float32(np.sqrt(np.sum(A[0, :3].astype(np.float64) ** 2)))
        inv = np.float32(1.0 / np.float64(scw))
        R = (A[:, :3] * inv).astype(np.float32); t = (A[:, 3] * inv).astype(np.float32)
        Ow = np.array([np.float32(-sum(np.float64(R[k, r]) * np.float64(t[k]) for k in range(3))) for r in range(3)], np.float32)
        assert np.array_equal(fs.decompose_scw(S).view(np.uint32), np.concatenate([R.ravel(), t, Ow]).view(np.uint32))


def test_disc_windows_hold_the_planted_candidate_counts():
    pl = disc()
    got = fs.fuse_sim3_eval_host(pl.scene(), want_cand=True)
    assert got["n_cand"][:, 7].tolist() == list(DISC_SIZES)      # the level-7 window holds the whole disc
    big = got["n_cand"][len(DISC_SIZES) - 1]
    assert big[0] < big[1] < big[2] < big[3] == 300 and big[2] > 256 and 0 < big[12] < big[8] < big[0]      # r = 4, 4.8, 5.76, 6.9 px; parts of the disc off the axis


def walk(batch, sc, s, S16, frames, which, rlib, table):
    """Eight resolve calls between which the map changes.  Of the points a call fuses, every third keeps living with the fused feature's descriptor (one outcome of
    ComputeDistinctiveDescriptors after Replace), every other third is skipped from then on (it is in a keyframe or replaced: isBad() || spAlreadyFound), and a few
    more points turn bad.  Every call must equal the reference's Fuse run with the current descriptors, compared on the points that are not skipped."""
    rng = np.random.default_rng(77)
    P = sc.P
    snapshot = s["pdesc"].copy(); now = snapshot.copy()
    skip = np.zeros(P, np.uint8)
    t = fs.unpack_table(table)
    n_reeval = 0; changed_seen = []; differs = 0
    for k in range(sc.K):
        nf, best, valid, _, _, _ = ref_fuse(rlib, frames, s, S16, which, k, pdesc=now)
        live = skip == 0
        changed = (now != snapshot).any(1)
        n, bi, bd = batch.resolve(k, skip, now)
        assert np.array_equal(bi[live], best[live]), k
        assert n == int((best[live] >= 0).sum()), k
        assert (bi[~live] == -1).all()
        n_reeval += int((changed & live & (valid > 0)).sum())
        assert batch.n_reeval() == n_reeval, k
        changed_seen.append(int((changed & live).sum()))
        stale = np.where(t["status"][k] == 7, t["idx"][k], -1)
        differs += int((stale[live] != bi[live]).any())
        fused = np.flatnonzero(live & (bi >= 0))
        kdesc = frames[which[k]][1]
        now[fused[0::3]] = kdesc[bi[fused[0::3]]]
        skip[fused[1::3]] = 1
        skip[rng.choice(P, 15, replace=False)] = 1
    assert sum(c >= 50 for c in changed_seen) >= 2, changed_seen
    assert differs >= 1


@needs_ref
def test_mirror_with_the_host_evaluator_through_eight_fuse_calls(frames, mixed, refs):
    sc, s, S16, which, got = mixed
    batch = fs.SearchAndFuseBatch(None, sc)
    try:
        tb = batch.table()
        assert np.array_equal(tb["table"], got["table"]) and np.array_equal(tb["n_hit"], got["n_hit"]) and np.array_equal(tb["n_valid"], got["n_valid"])
        walk(batch, sc, s, S16, frames, which, refs[0], got["table"])
    finally:
        batch.close()


def _bad(sc, **over):
    """a copy of the scene's arrays with some replaced"""
    import copy
    b = copy.copy(sc)
    for k, v in over.items():
        setattr(b, k, v)
    return b


def bad_argument_cases():
    """(name, scene) for every CCM_E_ARG rule of ccm_fuse_sim3_eval"""
    sc = fs.make_scene(3, 20, n_feat=40, seed=2)
    out = []
    off = sc.feat_off.copy(); off[1] = off[2] + 1
    out.append(("feat_off decreases", _bad(sc, feat_off=off)))
    off = sc.feat_off.copy(); off[0] = 1
    out.append(("feat_off does not start at 0", _bad(sc, feat_off=off)))
    co = sc.cell_off.copy(); j = int(np.flatnonzero(np.diff(co[:fs.CELLS + 1]) > 0)[0]); co[j + 1] = co[j] - 1
    out.append(("cell_off decreases", _bad(sc, cell_off=co)))
    co = sc.cell_off.copy(); co[0] = 1
    out.append(("cell_off does not start at 0", _bad(sc, cell_off=co)))
    co = sc.cell_off.copy(); co[2 * (fs.CELLS + 1) - 1] -= 1
    out.append(("cell_off ends short of the feature count", _bad(sc, cell_off=co)))
    ci = sc.cell_idx.copy(); ci[45] = 40
    out.append(("cell_idx out of range", _bad(sc, cell_idx=ci)))
    ci = sc.cell_idx.copy(); ci[0] = -1
    out.append(("cell_idx negative", _bad(sc, cell_idx=ci)))
    out.append(("nlevels 0", _bad(sc, nlevels=0)))
    out.append(("nlevels 17", _bad(sc, nlevels=17, scale_factors=np.ones(17, np.float32))))
    for name, th in (("th 0", 0.0), ("th negative", -1.0), ("th NaN", float("nan")), ("th Inf", float("inf"))):
        out.append((name, _bad(sc, th=th)))
    # more than 65 535 features in a keyframe
    n = 65536
    big = fs.Scene(sc.rec[:10], [0, n], np.zeros(2 * n, np.float32) + 100, np.zeros(n, np.uint8), np.zeros(32 * n, np.uint8),
                   np.concatenate([np.zeros(fs.CELLS, np.int32), [n]]), np.arange(n, dtype=np.int32) % 65535, sc.Scw[:12], sc.scale_factors, sc.log_sf, sc.th, sc.pos,
                   sc.normal, sc.min_dist, sc.max_dist, sc.pt_desc)
    out.append(("65 536 features", big))
    return out


def huge_product_case():
    """K * P beyond INT32_MAX: 65 536 x 32 768.  The rule is checked before any array is read, so the arrays stay those of a 1 x 1 scene."""
    return _bad(fs.make_scene(1, 1, n_feat=4, seed=1), K=65536, P=32768)


def test_every_bad_argument_is_refused_by_the_host_evaluator():
    h = fs._host()
    for name, b in bad_argument_cases():
        table = np.zeros(max(b.K * b.P, 1), np.uint32); nv = np.zeros(b.K, np.int32); nh = np.zeros(b.K, np.int32)
        assert h.ccmh_fuse_sim3_eval_host(*b.args(), fs._p(table), fs._p(nv), fs._p(nh), None, None) == -1, name
        with pytest.raises(CcmError):
            fs.SearchAndFuseBatch(None, b)
    b = huge_product_case()
    nv = np.zeros(b.K, np.int32); nh = np.zeros(b.K, np.int32); table = np.zeros(1, np.uint32)
    assert h.ccmh_fuse_sim3_eval_host(*b.args(), fs._p(table), fs._p(nv), fs._p(nh), None, None) == -1


def test_empty_calls_and_a_keyframe_without_features_are_legal():
    sc = fs.make_scene(3, 20, n_feat=40, seed=2)
    none = sc.subset([], 20)
    assert none.K == 0 and fs.fuse_sim3_eval_host(none)["table"].size == 0
    nopts = sc.subset([0, 1], 0)
    got = fs.fuse_sim3_eval_host(nopts)
    assert got["table"].shape == (2, 0) and not got["n_valid"].any()
    pl = planted()
    got = fs.fuse_sim3_eval_host(pl.scene())
    t = fs.unpack_table(got["table"])
    assert (t["status"][0] <= 4).all() and (t["status"][0] == 4).any() and got["n_hit"][0] == 0      # keyframe 0 has no features
    b = fs.SearchAndFuseBatch(None, none)
    assert b.table()["table"].size == 0
    b.close()
