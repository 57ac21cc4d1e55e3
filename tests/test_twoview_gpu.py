"""GPU: ccm_twoview_ransac_eval and ccm_twoview_check_rt (csrc/twoview.hip) against the host evaluator (the same twoview_math.h compiled with g++, which
tests/test_twoview_cpu.py pins to an independent numpy replay) — bit-identical scores, models, masks, statuses, points and cosines, no tolerance: every
operation is an IEEE add, multiply, divide or square root in f32 or f64 — the planted gates, the argument errors, two threads and the host mirror on the device."""
import ctypes as C
import threading

import numpy as np
import pytest

from test_triangulate_cpu import same_bits
from test_twoview_cpu import check_mirror

f32 = np.float32
SIZES_N = (8, 9, 31, 32, 33, 64, 65, 1000)
SIZES_H = (1, 2, 63, 64, 65, 200)


def tv():
    from ccm_slam_amd import twoview
    return twoview


def same_ransac(got, want, tag):
    for k, name in enumerate(("scoreH", "scoreF", "H21", "F21")):
        assert same_bits(got[k], want[k]), (tag, name)
    assert np.array_equal(got[4], want[4]) and np.array_equal(got[5], want[5]), (tag, "masks")


def same_rt(got, want, tag):
    assert np.array_equal(got[0], want[0]), (tag, "status", np.argwhere(got[0] != want[0])[:5])
    assert same_bits(got[1], want[1]) and same_bits(got[2], want[2]), tag


@pytest.fixture(scope="module")
def scenes():
    """one scene per size, with unmatched keypoints and a share of outliers, and its arguments; computed once"""
    out = {}
    for i, N in enumerate(SIZES_N):
        sc = tv().make_scene("general" if i % 2 else "planar", N, seed=50 + i, unmatched=N // 4, outliers=0.15 if N > 9 else 0.0)
        out[N] = (sc, tv().ransac_inputs(sc))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("N", SIZES_N)
def test_ransac_on_the_device_equals_the_host_evaluator(ctx, scenes, N):
    sc, a = scenes[N]
    for H in SIZES_H:
        sets = tv().random_sets(N, H, 1000 * N + H)
        got = tv().ransac_eval(ctx, *a, 1.0, sets)
        same_ransac(got, tv().ransac_eval_host(*a, 1.0, sets), (N, H))
        assert got[4].shape == (H, N)
    if N >= 64:                                                          # the scores separate the models of a good set from the rest
        assert got[0].max() > 0.5 * 5.991 * N or got[1].max() > 0.5 * 5.991 * N


@pytest.mark.gpu
def test_check_rt_on_the_device_equals_the_host_evaluator(ctx, scenes):
    seen = np.zeros(8, np.int64)
    for N in SIZES_N:
        sc, _ = scenes[N]
        inl = np.random.default_rng(N).random(N) < 0.9
        for n_hyp in (1, 4, 8):
            Rs, ts = tv().motion_hypotheses(sc, n_hyp)
            rec = np.stack([tv().prepare_rt(sc["K"], Rs[q], ts[q]) for q in range(n_hyp)])
            for th2 in (4.0, 0.5):
                got = tv().check_rt(ctx, rec, sc["K"], sc["xy1"], sc["xy2"], inl, th2)
                same_rt(got, tv().check_rt_host(rec, sc["K"], sc["xy1"], sc["xy2"], inl, th2), (N, n_hyp, th2))
                seen += np.bincount(got[0].reshape(-1), minlength=8)
    # NaN / Inf keypoints: a NaN keypoint gives a non-finite point, status 1 (an infinite one may still pass the SVD as a finite point)
    sc, _ = scenes[64]
    xy1 = sc["xy1"].copy(); xy2 = sc["xy2"].copy()
    xy1[3, 0] = np.nan; xy2[7, 1] = np.inf; xy1[11] = -np.inf; xy2[12] = np.nan
    Rs, ts = tv().motion_hypotheses(sc, 8)
    rec = np.stack([tv().prepare_rt(sc["K"], Rs[q], ts[q]) for q in range(8)])
    got = tv().check_rt(ctx, rec, sc["K"], xy1, xy2, np.ones(64, bool), 4.0)
    same_rt(got, tv().check_rt_host(rec, sc["K"], xy1, xy2, np.ones(64, bool), 4.0), "NaN / Inf keypoints")
    assert (got[0][:, [3, 12]] == 1).all()
    seen += np.bincount(got[0].reshape(-1), minlength=8)
    assert (seen > 0).all(), seen                                        # all eight status values
    # a mask with no inlier: status 0 and NaN everywhere
    got = tv().check_rt(ctx, rec, sc["K"], sc["xy1"], sc["xy2"], np.zeros(64, bool), 4.0)
    assert (got[0] == 0).all() and np.isnan(got[1]).all() and np.isnan(got[2]).all()


@pytest.mark.gpu
def test_degenerate_sets_and_non_finite_keypoints(ctx, scenes):
    sc, a = scenes[33]
    a = [np.array(x, copy=True) for x in a]
    N = 33
    # matches 0..3 coincide, 8..15 are collinear in both images, 16..23 are one single point: rank-deficient systems, the completion path
    for k in (0, 1, 2, 3):
        for x in a[:4]:
            x[k] = x[0]
    line = np.linspace(-1, 1, 8, dtype=f32)
    a[2][8:16] = np.stack([line, 0.5 * line], 1); a[3][8:16] = np.stack([0.9 * line, 0.45 * line + 0.1], 1)
    a[2][16:24] = a[2][16]; a[3][16:24] = a[3][16]
    sets = np.array([[0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 10, 11, 12, 13, 14, 15], [16, 17, 18, 19, 20, 21, 22, 23], [0, 1, 2, 3, 8, 9, 16, 17],
                     [15, 14, 13, 12, 11, 10, 9, 8], [24, 25, 26, 27, 28, 29, 30, 31]], np.int32)
    got = tv().ransac_eval(ctx, *a, 1.0, sets)
    same_ransac(got, tv().ransac_eval_host(*a, 1.0, sets), "degenerate sets")
    # normalised points that are all zero: both systems have rank <= 1
    z = [a[0], a[1], np.zeros_like(a[2]), np.zeros_like(a[3])] + a[4:]
    same_ransac(tv().ransac_eval(ctx, *z, 1.0, sets), tv().ransac_eval_host(*z, 1.0, sets), "zero points")
    # NaN / Inf keypoints, in the scored matches and in the sets
    b = [np.array(x, copy=True) for x in scenes[65][1]]
    b[0][5, 0] = np.nan; b[1][9, 1] = np.inf; b[2][20] = np.nan; b[3][21, 0] = -np.inf
    sets = tv().random_sets(65, 64, 3)
    got = tv().ransac_eval(ctx, *b, 1.0, sets)
    same_ransac(got, tv().ransac_eval_host(*b, 1.0, sets), "non-finite keypoints")
    assert np.isnan(got[0]).all()                                        # a NaN match poisons every sequential sum


def _plant_chi(target):
    """(d, sigma): a distance and a sigma with f32(f32(d * d) * f32(1.0 / (sigma * sigma))) == target; scanned over floats around sqrt(target) * sigma"""
    for sigma in (f32(1.0), f32(1.25), f32(0.8), f32(1.5), f32(0.7), f32(1.1)):
        inv = f32(1.0 / np.float64(sigma * sigma))
        d0 = f32(np.sqrt(float(target)) * float(sigma))
        d = d0 + np.arange(-3000, 3001, dtype=np.float64) * float(np.spacing(d0))
        d = d.astype(f32)
        chi = ((d * d).astype(f32) * inv).astype(f32)
        hit = np.nonzero(chi == target)[0]
        if hit.size:
            return d[hit[0]], sigma
    raise RuntimeError(f"no distance gives chi2 = {target!r}")


@pytest.mark.gpu
def test_planted_chi2_on_the_threshold_floats(ctx):
    """A match whose chi2 is the threshold float and its two neighbours, for both models, through the score hook.  H = I: chi2 = (u1 - u2)^2 / sigma^2 both
    ways; F of a pure x translation: chi2 = (v1 - v2)^2 / sigma^2 both ways."""
    I3 = np.eye(3, dtype=f32)
    Fx = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)
    for model, M, th, thScore in ((0, I3, f32(5.991), f32(5.991)), (1, Fx, f32(3.841), f32(5.991))):
        for target in (np.nextafter(th, f32(0)), th, np.nextafter(th, f32(10))):
            d, sigma = _plant_chi(target)
            xy1 = np.array([[10.0, 20.0], [d, d]], f32) if model == 0 else np.array([[10.0, 20.0], [7.0, d]], f32)
            xy2 = np.array([[10.0, 20.0], [0.0, d]], f32) if model == 0 else np.array([[-3.0, 20.0], [5.0, 0.0]], f32)
            score, mask = tv().score_device(ctx, model, M[None], xy1, xy2, sigma)
            hs, hm = tv().score_host(model, M[None], xy1, xy2, sigma)
            assert same_bits(score, hs) and np.array_equal(mask, hm), (model, target)
            inside = not target > th
            assert mask[0, 0] and mask[0, 1] == inside, (model, target, mask)
            term = thScore - target if inside else f32(0)                # match 0 adds thScore twice, match 1 its term twice
            assert score[0] == f32(f32(f32(thScore + thScore) + term) + term), (model, target, score)


@pytest.mark.gpu
def test_planted_parallax_threshold_and_a_point_at_the_second_centre(ctx):
    K = tv().K_matrix()
    rec = tv().prepare_rt(K, np.eye(3), [-0.3, 0, 0])
    # keypoint 1 on the principal point, keypoint 2 scanned float by float around the disparity of a point 47 deep: cosParallax crosses 0.99998
    x0 = f32(K[0, 2] - K[0, 0] * 0.3 / 47.4)
    xs = (x0 + np.arange(-6000, 6001, dtype=np.float64) * float(np.spacing(x0))).astype(f32)
    xy1 = np.tile(np.array([[K[0, 2], K[1, 2]]], f32), (xs.size, 1))
    xy2 = np.stack([xs, np.full(xs.size, K[1, 2], f32)], 1)
    inl = np.ones(xs.size, bool)
    host = tv().check_rt_host(rec[None], K, xy1, xy2, inl, 4.0)
    c0 = f32(0.99998)
    pick = []
    for want in (np.nextafter(c0, f32(0)), c0, np.nextafter(c0, f32(2))):
        hit = np.nonzero(host[2][0] == want)[0]
        assert hit.size, f"no keypoint gives cos = {want!r}"
        pick.append(int(hit[0]))
    got = tv().check_rt(ctx, rec[None], K, xy1[pick], xy2[pick], np.ones(3, bool), 4.0)
    same_rt(got, tuple(x[:, pick] for x in host), "parallax threshold")
    assert [int(s) for s in got[0][0]] == [7 if float(c) < 0.99998 else 6 for c in got[2][0]]   # the float promoted to double against the double constant
    assert 6 in got[0][0] and 7 in got[0][0]
    same_rt(tv().check_rt(ctx, rec[None], K, xy1, xy2, inl, 4.0), host, "the whole scan")
    # a record whose O2 is the triangulated point itself: normal2 = 0, dist2 = 0, cosParallax = 0 / 0; the match is counted with low parallax
    sc = tv().make_scene("general", 8, seed=70)
    Rs, ts = tv().motion_hypotheses(sc, 1)
    rec = tv().prepare_rt(sc["K"], Rs[0], ts[0])
    first = tv().check_rt(ctx, rec[None], sc["K"], sc["xy1"], sc["xy2"], np.ones(8, bool), 4.0)
    k = int(np.nonzero(first[0][0] == 7)[0][0])
    rec2 = rec.copy(); rec2[12:15] = first[1][0, k]
    got = tv().check_rt(ctx, rec2[None], sc["K"], sc["xy1"], sc["xy2"], np.ones(8, bool), 4.0)
    same_rt(got, tv().check_rt_host(rec2[None], sc["K"], sc["xy1"], sc["xy2"], np.ones(8, bool), 4.0), "a point at O2")
    assert got[0][0, k] == 6 and np.isnan(got[2][0, k]) and same_bits(got[1][0, k], first[1][0, k])


@pytest.mark.gpu
def test_error_paths(ctx, scenes):
    from ccm_slam_amd._lib import CcmError, lib
    sc, a = scenes[9]
    sets = tv().random_sets(9, 3, 0)
    tv().ransac_eval(ctx, *a, 1.0, sets)
    for i, j, v in ((0, 0, -1), (1, 7, 9), (2, 3, None)):                # an index below 0, one at N, one repeated within its set
        bad = sets.copy(); bad[i, j] = bad[i, (j + 1) % 8] if v is None else v
        with pytest.raises(CcmError):
            tv().ransac_eval(ctx, *a, 1.0, bad)
    with pytest.raises(CcmError):                                        # N < 8
        tv().ransac_eval(ctx, *[x[:7] for x in a[:4]], *a[4:], 1.0, np.arange(8, dtype=np.int32)[None] % 7)
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)
    keep = [np.ascontiguousarray(x, f32) for x in a] + [np.ascontiguousarray(sets)]
    o = [np.zeros(3, f32), np.zeros(3, f32), np.zeros(27, f32), np.zeros(27, f32), np.zeros(3, np.uint32), np.zeros(3, np.uint32)]
    full = [9] + [p(x) for x in keep[:7]] + [C.c_float(1.0), 3, p(keep[7])] + [p(x) for x in o]
    assert lib().ccm_twoview_ransac_eval(ctx.handle, *full) == 0
    for i in (1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14, 15, 16):          # each pointer in turn
        b = list(full); b[i] = None
        assert lib().ccm_twoview_ransac_eval(ctx.handle, *b) == -1, i
    b = list(full); b[9] = 0                                             # H < 1
    assert lib().ccm_twoview_ransac_eval(ctx.handle, *b) == -1
    b = list(full); b[0] = 7                                             # N < 8
    assert lib().ccm_twoview_ransac_eval(ctx.handle, *b) == -1
    assert lib().ccm_twoview_ransac_eval(None, *full) == -1
    # ccm_twoview_check_rt
    Rs, ts = tv().motion_hypotheses(sc, 8)
    rec = np.ascontiguousarray(np.stack([tv().prepare_rt(sc["K"], Rs[q], ts[q]) for q in range(8)]))
    Kk = np.ascontiguousarray(sc["K"]); mask = np.array([0x1ff], np.uint32)
    st = np.zeros(72, np.uint8); x = np.zeros(216, f32); cp = np.zeros(72, f32)
    full = [8, p(rec), p(Kk), 9, p(keep[0]), p(keep[1]), p(mask), C.c_float(4.0), p(st), p(x), p(cp)]
    assert lib().ccm_twoview_check_rt(ctx.handle, *full) == 0
    for i in (1, 2, 4, 5, 6, 8, 9, 10):
        b = list(full); b[i] = None
        assert lib().ccm_twoview_check_rt(ctx.handle, *b) == -1, i
    for i, v in ((0, 0), (0, 9), (3, 0)):                                # n_hyp outside [1, 8], N < 1
        b = list(full); b[i] = v
        assert lib().ccm_twoview_check_rt(ctx.handle, *b) == -1, (i, v)
    assert lib().ccm_twoview_check_rt(None, *full) == -1
    assert lib().ccm_twoview_check_rt(ctx.handle, *full) == 0            # the context still works after the refusals


@pytest.mark.gpu
def test_two_threads_with_their_own_contexts_and_reruns(scenes):
    from ccm_slam_amd._lib import Context
    jobs = []
    for N, H in ((65, 200), (1000, 65)):
        sc, a = scenes[N]
        sets = tv().random_sets(N, H, N)
        Rs, ts = tv().motion_hypotheses(sc, 8)
        rec = np.stack([tv().prepare_rt(sc["K"], Rs[q], ts[q]) for q in range(8)])
        inl = np.ones(N, bool)
        jobs.append((a, sets, rec, sc, inl, tv().ransac_eval_host(*a, 1.0, sets), tv().check_rt_host(rec, sc["K"], sc["xy1"], sc["xy2"], inl, 4.0)))
    out = [None, None]
    err = []

    def worker(i):
        try:
            a, sets, rec, sc, inl, _, _ = jobs[i]
            c = Context(0)
            out[i] = [(tv().ransac_eval(c, *a, 1.0, sets), tv().check_rt(c, rec, sc["K"], sc["xy1"], sc["xy2"], inl, 4.0)) for _ in range(4)]
            c.close()
        except Exception as e:   # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for i in range(2):
        for r, c in out[i]:                                              # every run, the first included, is the host evaluator's answer bit for bit
            same_ransac(r, jobs[i][5], ("thread", i)); same_rt(c, jobs[i][6], ("thread", i))


@pytest.mark.gpu
def test_mirror_on_the_device_equals_the_literal_sequence():
    check_mirror(0, lambda a, sigma, sets: tv().ransac_eval_host(*a, sigma, sets), tv().check_rt_host, cases=(("planar", 120, 31), ("general", 77, 32)))
