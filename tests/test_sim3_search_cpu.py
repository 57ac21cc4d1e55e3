"""ComputeSim3's two projected searches on the CPU: csrc/fuse_math.h compiled by g++ (libccm_host.so) against the reference's own
ORBmatcher::SearchByProjection(pKF, Scw, ...) and ORBmatcher::SearchBySim3 (oracle/_ref/libmatcher_ref.so through ref_search_by_projection_sim3 and
ref_search_by_sim3), against oracle.projected_window_search, against Fuse's evaluator with the mask off, and against hand-made pairs with known answers; the mirrors
cslam::Sim3ProjectionSearch and cslam::SearchBySim3Batch with the host evaluator on a host-only keyframe store; ssm_derive against a numpy-scalar restatement; every
bad-argument rule.  Every comparison is exact: integers, and float bit patterns."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import tests.test_ref_matcher as trm
from ccm_slam_amd import fuse_sim3 as fs, sim3_search as ss, synth
from ccm_slam_amd._lib import CcmError
from ccm_slam_amd.kfstore import KeyFrameStore
from fuse_sim3_cases import DISC_SIZES, disc, planted, scene_from_frames
from sim3_search_cases import (angle_rejected_by_fuse, expected_reeval, pair_all_points, pair_case, pair_keyframes, pair_planted, pair_sides, projection_case,
                               projection_scene, ref_pair, ref_projection, same_gates_as_reference)

needs_ref = pytest.mark.skipif(not os.path.exists(trm.LIB) and not os.path.isdir("/root/reference/cslam"), reason="oracle/_ref not built")
f32 = np.float32


@pytest.fixture(scope="module")
def frames():
    o = oracle.OrbOracle(1000)
    out = [o.extract(synth.gen_image(1000, t)) for t in (0, 1)]
    o.close()
    return out


@pytest.fixture(scope="module")
def rlib():
    if not os.path.exists(trm.LIB):
        from oracle import ref
        ref.build()
    return C.CDLL(trm.LIB)


@pytest.fixture(scope="module")
def proj(frames):
    """the projection case, and per th the scene and the host evaluator's table on the initial mask, computed once"""
    case = projection_case(frames)
    out = {}
    for th in (10, 4):
        sc = projection_scene(frames, case, th)
        out[th] = (sc, ss.project_eval_host(sc, [case["matched0"] >= 0], want_uv=True))
    return case, out


def host_store(sc, keys):
    st = KeyFrameStore(None, max(len(keys), 1), 2048)
    st.add_scene(keys, sc, grid=True)
    return st


# ---- 1, 2: the projection scene ------------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("th", (10, 4))
def test_projection_scene_against_the_references_search_by_projection(frames, rlib, proj, th):
    case, by_th = proj
    sc, got = by_th[th]
    s = case["s"]; kps = s["kps"]
    n, ref_matched, valid, u, v, lvl = ref_projection(rlib, case, th)
    # the reference alone
    en, ebi, _, _ = oracle.projected_window_search(kps["x"], kps["y"], kps["octave"], s["desc"], trm.BOUNDS, s["sf"], s["isig"], valid, u, v, lvl, s["pdesc"], float(th),
                                                   False, 50, matched=case["matched0"], claim=True, no_claim=case["no_claim"])
    remapped = int(((ebi >= 0) & (case["no_claim"] > 0)).sum())
    assert n > 600 and remapped > 30 and n == en - remapped
    # the host table's gates
    t = fs.unpack_table(got["table"][0]); uv = got["uv"][0]
    m = valid > 0
    assert np.array_equal(t["status"] >= 4, m)
    assert np.array_equal(uv[m, 0].view(np.uint32), u[m].view(np.uint32)) and np.array_equal(uv[m, 1].view(np.uint32), v[m].view(np.uint32))
    assert np.array_equal(t["level"][m], lvl[m])
    # the mirror with the host evaluator
    st = host_store(sc, [70])
    srch = ss.Sim3ProjectionSearch(st, 70, sc, case["matched0"] >= 0)
    assert np.array_equal(srch.table()["table"], got["table"][0])
    nm, matched, best, remap = srch.resolve(case["matched0"], None, case["existing"])
    assert nm == n and np.array_equal(matched, ref_matched)
    assert int((remap >= 0).sum()) == remapped and not ((remap >= 0) & (case["existing"] < 0)).any()
    assert np.array_equal(np.flatnonzero(best >= 0), np.sort(matched[(matched >= 0) & (matched < 1_000_000)]))
    exp = expected_reeval(got["table"][0], None, matched)
    assert exp > 0 and srch.n_reeval() == exp


@pytest.mark.parametrize("th", (10, 4))
def test_initial_state_table_against_the_oracles_window_search(proj, th):
    case, by_th = proj
    sc, got = by_th[th]
    s = case["s"]; kps = s["kps"]
    t = fs.unpack_table(got["table"][0]); uv = got["uv"][0]
    valid = (t["status"] >= 4).astype(np.uint8)
    en, ebi, _, _ = oracle.projected_window_search(kps["x"], kps["y"], kps["octave"], s["desc"], trm.BOUNDS, s["sf"], s["isig"], valid, uv[:, 0], uv[:, 1], t["level"],
                                                   s["pdesc"], float(th), False, 50, matched=case["matched0"], claim=False)
    hit = t["status"] == 7
    assert en == int(hit.sum()) == got["n_hit"][0] and en > 600
    assert np.array_equal(hit, ebi >= 0) and np.array_equal(t["idx"][hit], ebi[hit])
    # the mask matters here: without it more points hit, and none of the masked features is ever an answer
    free = fs.unpack_table(ss.project_eval_host(sc)["table"][0])
    assert (free["status"] == 7).sum() > en and not (case["matched0"][t["idx"][hit]] >= 0).any()


# ---- 3: mask off equals Fuse ---------------------------------------------------------------------------------------------------------------
def test_mask_off_equals_fuse(frames):
    for sc in (planted().scene(), disc().scene(), scene_from_frames(frames, "nnffnnff")[0]):
        a = fs.fuse_sim3_eval_host(sc, want_uv=True)
        b = ss.project_eval_host(sc, want_uv=True)
        assert np.array_equal(a["table"], b["table"]) and np.array_equal(a["uv"].view(np.uint32), b["uv"].view(np.uint32))
        assert np.array_equal(a["n_valid"], b["n_valid"]) and np.array_equal(a["n_hit"], b["n_hit"])


# ---- 4: planted masks ------------------------------------------------------------------------------------------------------------------------
def planted_mask_cases():
    """(scene, masks, {(k, i): (status, idx, dist)}) with known answers, on the keyframes of fuse_sim3_cases.planted()"""
    pl = planted()
    sc = pl.scene()
    counts = np.diff(sc.feat_off)
    masks = [np.zeros(n, np.uint8) for n in counts]
    exp = {}
    one = [k for k in range(sc.K) if counts[k] == 1]
    hits = [(k, i) for (k, i), e in pl.expect.items() if e[0] == 7 and counts[k] == 1]
    assert len(hits) >= 6
    for k, i in hits:                      # the single feature under the projection masked: in the window, no candidate -> 5, not 4
        masks[k][0] = 1
        exp[k, i] = (5, -1, -1)
    # the ties: the earlier of two equal candidates masked -> the later wins
    ties = [(k, i, e) for (k, i), e in pl.expect.items() if counts[k] == 4 and e[0] == 7]
    assert len(ties) == 3
    for k, i, e in ties:
        masks[k][e[1]] = 1
        exp[k, i] = (7, 4 - e[1], 9)       # features 1 and 3 tie
    assert one
    return sc, masks, exp


def test_planted_masks():
    sc, masks, exp = planted_mask_cases()
    t = fs.unpack_table(ss.project_eval_host(sc, masks)["table"])
    for (k, i), (st, idx, dist) in exp.items():
        assert (int(t["status"][k, i]), int(t["idx"][k, i]), int(t["dist"][k, i])) == (st, idx, dist), (k, i)


def disc_masks(sc):
    return [(np.arange(n) % 2).astype(np.uint8) for n in np.diff(sc.feat_off)]


def disc_expected(sc, masks, got, k):
    """keyframe k's row by a numpy arg-min over the unmasked candidates, in the order oracle.grid_candidates gives (the reference's): [(status, idx, dist)]"""
    a, b = int(sc.feat_off[k]), int(sc.feat_off[k + 1])
    xy = sc.feat_xy.reshape(-1, 2)[a:b]; oc = sc.feat_octave[a:b].astype(np.int32); de = sc.feat_desc.reshape(-1, 32)[a:b]
    t = fs.unpack_table(got["table"][k])
    u, v, lvl = got["uv"][k, :, 0], got["uv"][k, :, 1], t["level"].astype(np.int32)
    r = (f32(sc.th) * sc.scale_factors[lvl]).astype(np.float32)
    none = -np.ones(sc.P, np.int32)
    aoff, _ = oracle.grid_candidates(xy[:, 0], xy[:, 1], oc, trm.BOUNDS, u, v, r, none, none)
    loff, lidx = oracle.grid_candidates(xy[:, 0], xy[:, 1], oc, trm.BOUNDS, u, v, r, lvl - 1, lvl)
    bits = np.unpackbits(de, axis=1).astype(np.int16) if b > a else np.zeros((0, 256), np.int16)
    out = []
    for i in range(sc.P):
        cand = [f for f in lidx[loff[i]:loff[i + 1]] if not masks[k][f]]
        if aoff[i + 1] == aoff[i]:
            out.append((4, -1, -1))
        elif not cand:
            out.append((5, -1, -1))
        else:
            d = np.abs(bits[cand] - np.unpackbits(sc.pt_desc.reshape(-1, 32)[i]).astype(np.int16)).sum(1)
            j = int(np.argmin(d))                   # the first minimum, in the reference's candidate order
            out.append((7 if d[j] <= 50 else 6, int(cand[j]), int(d[j])))
    return out


def test_disc_with_odd_features_masked_against_a_numpy_arg_min():
    sc = disc().scene()
    assert tuple(np.diff(sc.feat_off)) == DISC_SIZES
    masks = disc_masks(sc)
    got = ss.project_eval_host(sc, masks, want_uv=True)
    t = fs.unpack_table(got["table"])
    seen = set()
    for k in range(sc.K):
        assert (t["status"][k] >= 4).all()
        exp = disc_expected(sc, masks, got, k)
        for i in range(sc.P):
            assert (int(t["status"][k, i]), int(t["idx"][k, i]), int(t["dist"][k, i])) == exp[i], (k, i)
            seen.add(exp[i][0])
            assert exp[i][1] < 0 or exp[i][1] % 2 == 0
    assert {4, 5, 7} <= seen
    # the masks change answers in this scene
    assert not np.array_equal(got["table"], ss.project_eval_host(sc)["table"])


# ---- 5: ssm_derive ---------------------------------------------------------------------------------------------------------------------------
def test_ssm_derive_against_a_numpy_scalar_restatement():
    rng = np.random.default_rng(3)
    for it in range(50):
        s12 = f32(1.0) if it == 0 else f32(rng.uniform(0.3, 3.0))
        R = synth.rodrigues(rng.normal(0, 0.5, (1, 3)))[0].astype(np.float32).reshape(-1)
        t = rng.normal(0, 1, 3).astype(np.float32)
        a, b, cc = ss.derive(float(s12), R, t)
        e_a = np.array([f32(x * s12) for x in R], np.float32)                                   # Mat * s: the product in float
        alpha = f32(np.float64(1.0) / np.float64(s12))                                           # the double quotient rounded to float
        e_b = np.array([f32(R[3 * col + r] * alpha) for r in range(3) for col in range(3)], np.float32)
        e_c = np.zeros(3, np.float32)
        for r in range(3):
            n = [f32(-e_b[3 * r + k]) for k in range(3)]
            acc = f32(f32(f32(n[0] * t[0]) + f32(n[1] * t[1])) + f32(n[2] * t[2]))             # a float accumulator, left to right
            e_c[r] = f32(np.float64(acc) * 1.0 + 0.0)
        for got, exp in ((a, e_a), (b, e_b), (cc, e_c)):
            assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), it


# ---- 6: the pair scene ------------------------------------------------------------------------------------------------------------------------
@needs_ref
def test_pair_scene_against_the_references_search_by_sim3(frames, rlib):
    p = pair_case(frames)
    n, out12, d1, d2 = ref_pair(rlib, p)
    assert d1[0].sum() > 500 and d2[0].sum() > 500 and n > 300
    kfs = pair_keyframes(p)
    res = ss.pair_eval_host(pair_all_points(p, kfs), want_uv=True)
    same_gates_as_reference(res, 0, p["N"], p["has1"], d1, "1 -> 2")
    same_gates_as_reference(res, 1, p["N"], p["has2"], d2, "2 -> 1")
    st = host_store(kfs, [11, 12])
    s1, s2 = pair_sides(p)
    got = ss.search_by_sim3(st, 11, 12, s1, s2, p["s12"], p["R12"], p["t12"], p["pre12"], p["sf"], p["th"])
    assert got["nFound"] == n and np.array_equal(got["matches12"], out12)
    # the store's shadows give what the flat arrays give
    res2 = ss.pair_eval_resident_host(st, [11, 12], pair_all_points(p, kfs), want_uv=True)
    assert np.array_equal(res["table"], res2["table"]) and np.array_equal(res["uv"].view(np.uint32), res2["uv"].view(np.uint32))


# ---- 7: planted pairs -------------------------------------------------------------------------------------------------------------------------
def test_planted_pairs():
    pl = pair_planted()
    res = ss.pair_eval_host(pl.scene(), want_uv=True)
    pl.check(res)
    t = fs.unpack_table(res["table"])
    assert not (t["status"] == 3).any()
    for j in range(len(pl.jobs)):
        a, b = int(res["off"][j]), int(res["off"][j + 1])
        assert res["n_valid"][j] == (t["status"][a:b] >= 4).sum() and res["n_hit"][j] == (t["status"][a:b] == 7).sum()


def test_a_point_fuses_angle_gate_rejects_passes_the_pair_gate():
    pl = angle_rejected_by_fuse()
    sc = pl.scene()
    pl.check(fs.fuse_sim3_eval_host(sc)["table"])
    ps = ss.PairScene(sc, 4.0, sc.pos, sc.min_dist, sc.max_dist, sc.pt_desc, [(0, sc.rec[:4], np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32),
                                                                                np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32), 0, sc.P)])
    assert fs.unpack_table(ss.pair_eval_host(ps)["table"])["status"].tolist() == [4]


# ---- 8: bad arguments and empty calls ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_and_empty_calls_of_the_projection_entry():
    sc = planted().scene()
    counts = np.diff(sc.feat_off)
    st = host_store(sc, list(range(100, 100 + sc.K)))
    keys = list(range(100, 100 + sc.K))
    off, sk = ss.pack_masks([None] * sc.K, counts)
    ok = lambda **kw: (ss.project_eval_host(sc, **kw), ss.project_eval_resident_host(st, keys, sc, **kw))
    ok(skip=(off, sk))

    def bad(**kw):
        with pytest.raises(CcmError):
            ss.project_eval_host(sc, **kw)
        with pytest.raises(CcmError):
            ss.project_eval_resident_host(st, keys, sc, **kw)
    o = off.copy(); o[0] = 1
    bad(skip=(o, sk))                                                # does not start at 0
    o = off.copy(); k1 = int(np.flatnonzero(counts > 0)[0]); o[k1 + 1] = o[k1] - 1
    bad(skip=(o, np.zeros(sk.size + 8, np.uint8)))                   # decreases
    o = off.copy(); o[k1 + 1:] += 1
    bad(skip=(o, np.zeros(sk.size + 8, np.uint8)))                   # a mask longer than its keyframe's features
    o = off.copy(); o[-1] -= 1
    bad(skip=(o, sk))                                                # ... and shorter
    bad(skip=(None, sk))
    bad(skip=(off, None))
    # what ccm_fuse_sim3_eval_resident refuses
    for attr, val in (("nlevels", 0), ("nlevels", 17), ("th", 0.0), ("th", float("nan")), ("th", float("inf")), ("P", -1)):   # (P = -1 with the arrays of P points)
        old = getattr(sc, attr); setattr(sc, attr, val)
        try:
            bad(skip=(off, sk))
        finally:
            setattr(sc, attr, old)
    with pytest.raises(CcmError):
        ss.project_eval_resident_host(st, [100, 9999], sc.subset([0, 1]), skip=(np.zeros(3, np.int32), np.zeros(1, np.uint8)))   # a key that is not live
    # empty calls
    e = ss.project_eval_host(sc.subset([]), [])
    assert e["table"].size == 0 and e["n_valid"].size == 0
    e = ss.project_eval_resident_host(st, [], sc.subset([]), [])
    assert e["table"].size == 0
    e = ss.project_eval_resident_host(st, keys, sc.subset(range(sc.K), 0))
    assert e["table"].size == 0 and not e["n_valid"].any()
    # NaN and Inf are values, not errors: planted() holds them
    assert ss.project_eval_host(sc)["table"].shape == (sc.K, sc.P)


def test_bad_arguments_and_empty_calls_of_the_pair_entry():
    pl = pair_planted()
    ps = pl.scene()
    K = ps.kfs.K
    keys = list(range(200, 200 + K))
    st = host_store(ps.kfs, keys)
    jobs = list(pl.jobs)
    ref = ss.pair_eval_host(ps)
    assert np.array_equal(ref["table"], ss.pair_eval_resident_host(st, keys, ps)["table"])

    def bad():
        with pytest.raises(CcmError):
            ss.pair_eval_host(ps)
        with pytest.raises(CcmError):
            ss.pair_eval_resident_host(st, keys, ps)
    j0 = jobs[0]
    for broken in ((K,) + j0[1:], (-1,) + j0[1:], j0[:4] + (-1, 1), j0[:4] + (0, -1), j0[:4] + (ps.P, 1), j0[:4] + (1, ps.P)):
        ps.set_jobs([broken] + jobs[1:])
        bad()
    ps.set_jobs(jobs)
    for name in ("job_kf", "job_K4", "job_src", "job_T", "job_pt0", "job_n"):
        old = getattr(ps, name); setattr(ps, name, None)
        try:
            bad()
        finally:
            setattr(ps, name, old)
    for attr, val in (("nlevels", 0), ("nlevels", 17), ("th", -1.0), ("th", float("nan")), ("J", -1)):
        old = getattr(ps, attr); setattr(ps, attr, val)
        try:
            bad()
        finally:
            setattr(ps, attr, old)
    with pytest.raises(CcmError):
        ss.pair_eval_resident_host(st, keys[:-1] + [9999], ps)
    # empty calls: no jobs, an empty job, no points, no keyframes
    ps.set_jobs([])
    assert ss.pair_eval_host(ps)["table"].size == 0 and ss.pair_eval_resident_host(st, keys, ps)["table"].size == 0
    ps.set_jobs([j0[:4] + (0, 0)] + jobs[1:])
    e = ss.pair_eval_host(ps)
    assert e["n_valid"][0] == 0 and np.array_equal(e["table"], ref["table"][jobs[0][5]:])
    empty = ss.PairScene(ps.kfs, 4.0, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0, np.uint8), [j0[:4] + (0, 0)])
    assert ss.pair_eval_host(empty)["table"].size == 0 and ss.pair_eval_resident_host(st, keys, empty)["table"].size == 0
    none = ss.PairScene(ps.kfs.subset([]), 4.0, ps.pos, ps.min_dist, ps.max_dist, ps.pt_desc, [])
    assert ss.pair_eval_host(none)["table"].size == 0 and ss.pair_eval_resident_host(st, [], none)["table"].size == 0
