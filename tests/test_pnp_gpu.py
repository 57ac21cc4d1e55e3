"""GPU: ccm_pnp_ransac_eval and cslam::PnPRansacBatch on the device against the host evaluator (csrc/pnp_math.h compiled with g++; its own bits are checked
against a literal replay of PnPSolver.cpp in tests/test_pnp_cpu.py).  n_inl and the masks are equal, Rt is equal bit for bit where finite; where it is not finite
only the positions of the non-finite entries must agree (x86 and the device sign their default NaN differently).  Tail bits of every mask word are zero
(pnp._eval fills the mask with ones before the call and raises when a bit beyond N survives)."""
import numpy as np
import pytest

import pnp_cases as pc
from ccm_slam_amd import pnp, sim3
from ccm_slam_amd._lib import CcmError, _p, lib

pytestmark = pytest.mark.gpu


def _same(got, want, tag=""):
    (n, Rt, masks), (hn, hRt, hmasks) = got, want
    assert np.array_equal(n, hn), (tag, n, hn)
    assert len(masks) == len(hmasks) and all(np.array_equal(a, b) for a, b in zip(masks, hmasks)), tag
    fin, hfin = np.isfinite(Rt), np.isfinite(hRt)
    assert np.array_equal(fin, hfin), (tag, Rt[~fin | ~hfin], hRt[~fin | ~hfin])
    a = np.ascontiguousarray(Rt).view(np.uint64); b = np.ascontiguousarray(hRt).view(np.uint64)
    assert np.array_equal(a[fin], b[fin]), (tag, int((a[fin] != b[fin]).sum()), np.abs(Rt[fin] - hRt[fin]).max())


def _hyps(rng, cands, H, interleave=True):
    hc = (np.arange(H) % len(cands)).astype(np.int32) if interleave else np.sort(rng.integers(0, len(cands), H)).astype(np.int32)
    hi = np.array([rng.choice(cands[c].N, 4, replace=False) for c in hc], np.int32).reshape(-1, 4)
    return hc, hi


@pytest.mark.parametrize("N", [4, 5, 31, 32, 33, 63, 64, 65])
def test_one_candidate_at_the_wave_block_and_mask_word_edges(ctx, N):
    """H = 1 (one wave), 4 (a whole workgroup) and 5 (one wave in a second workgroup); N around the 32-bit mask words and the 64-lane stride."""
    c = pc.make_candidate(300 + N, max(4, (2 * N) // 3), N - max(4, (2 * N) // 3))
    rng = np.random.default_rng(N)
    for H in (1, 4, 5):
        hc, hi = _hyps(rng, [c], H)
        _same(pnp.eval_hypotheses(ctx, [c], hc, hi), pnp.eval_hypotheses_host([c], hc, hi), (N, H))


def test_three_candidates_with_their_own_intrinsics_and_thresholds(ctx):
    cands = [pc.make_candidate(41, 4, 0, cam=(500.0, 510.0, 320.0, 240.0)), pc.make_candidate(42, 25, 8, cam=(420.5, 415.25, 300.0, 220.0)),
             pc.make_candidate(43, 50, 20, cam=(700.0, 690.0, 640.0, 360.0))]
    assert [c.N for c in cands] == [4, 33, 70]
    rng = np.random.default_rng(4)
    for k, c in enumerate(cands):
        c.sigma2 = ((1.2 ** rng.integers(0, 8, c.N)) ** 2).astype(np.float32) * np.float32(1 + k)     # level sigmas, another range per candidate
    hc, hi = _hyps(rng, cands, 23)
    got = pnp.eval_hypotheses(ctx, cands, hc, hi)
    _same(got, pnp.eval_hypotheses_host(cands, hc, hi))
    assert got[0].max() >= 25       # a sample of true correspondences finds its candidate's inliers


def test_degenerate_samples(ctx):
    c = pc.make_candidate(51, 30, 6)
    P = np.array(c.P3Dw, np.float32)
    P[1] = P[0]                                             # two identical 3D points
    P[4:8, 2] = 5.0                                         # four coplanar points: the third PCA value is 0, CC is singular, cvInvert takes its pseudo-inverse path
    R, t = c.meta["R"], c.meta["t"]
    P[20] = (R.T @ (np.array([0.3, -0.2, 0.0]) - t)).astype(np.float32)    # a point on the camera plane of the true pose (Zc = 0 up to rounding)
    P[21] = (R.T @ (np.array([0.3, -0.2, -2.0]) - t)).astype(np.float32)   # a point behind the camera
    c.P3Dw = P
    true = np.nonzero(c.meta["true"] & (np.arange(c.N) > 21))[0]
    hi = np.array([[0, 1, 2, 3], [1, 0, 9, 10], [4, 5, 6, 7], [7, 6, 5, 4], [20, 2, 3, 9], [21, 2, 3, 9], true[:4], true[4:8]], np.int32)
    hc = np.zeros(len(hi), np.int32)
    got = pnp.eval_hypotheses(ctx, [c], hc, hi)
    _same(got, pnp.eval_hypotheses_host([c], hc, hi))
    for h in (6, 7):                                         # under a pose from true correspondences neither of the two points is an inlier
        assert not got[2][h][20] and not got[2][h][21]


def test_threshold_edge(ctx):
    from test_pnp_cpu import threshold_edge_candidates
    at, above, sample, i = threshold_edge_candidates()
    _, _, m_at = pnp.eval_hypotheses(ctx, [at], [0], [sample], th2=1.0)
    _, _, m_above = pnp.eval_hypotheses(ctx, [above], [0], [sample], th2=1.0)
    assert not m_at[0][i] and m_above[0][i]
    assert np.array_equal(np.delete(m_at[0], i), np.delete(m_above[0], i))


def test_argument_errors_and_the_empty_call(ctx):
    c = pc.make_candidate(61, 10, 2)
    ok = np.array([[0, 1, 2, 3]], np.int32)
    for hc, hi in (([0], [[0, 1, 2, 12]]), ([0], [[0, 1, 2, -1]]), ([0], [[0, 1, 2, 2]]), ([0], [[5, 1, 2, 5]]), ([1], ok), ([-1], ok)):
        with pytest.raises(CcmError):
            pnp.eval_hypotheses(ctx, [c], hc, hi)
        with pytest.raises(CcmError):
            pnp.eval_hypotheses_host([c], hc, hi)
    with pytest.raises(CcmError):                               # a candidate with N < 4
        pnp.eval_hypotheses(ctx, [c, pc.make_candidate(62, 3, 0)], [0], ok)
    # raw calls: K < 1, H < 0, null pointers
    pt_off, P3, P2, s2, cam, _, _ = pnp.pack([c])
    me = pnp.max_errors(s2)
    hc = np.zeros(1, np.int32); hi = ok.reshape(-1).copy(); n_inl = np.zeros(1, np.int32); Rt = np.zeros(12); mo = np.zeros(2, np.int32); mask = np.zeros(1, np.uint32)
    f = lib().ccm_pnp_ransac_eval
    good = [1, _p(pt_off), _p(P3), _p(P2), _p(me), _p(cam), 1, _p(hc), _p(hi), _p(n_inl), _p(Rt), _p(mo), _p(mask)]
    assert f(ctx.handle, *good) == 0 and n_inl[0] >= 0
    assert f(None, *good) == -1
    for pos, val in ((0, 0), (6, -1), (1, None), (2, None), (3, None), (4, None), (5, None), (7, None), (8, None), (9, None), (10, None), (11, None), (12, None)):
        a = list(good); a[pos] = val
        assert f(ctx.handle, *a) == -1, pos
    bad_off = np.array([1, 13], np.int32)
    a = list(good); a[1] = _p(bad_off)
    assert f(ctx.handle, *a) == -1
    # H = 0 succeeds, writes mask_off[0] and touches nothing else
    mo[:] = 7; n_inl[:] = -5
    a = list(good); a[6] = 0
    for k in (7, 8, 9, 10, 12):
        a[k] = None
    assert f(ctx.handle, *a) == 0 and mo[0] == 0 and mo[1] == 7 and n_inl[0] == -5
    n, Rt2, masks = pnp.eval_hypotheses(ctx, [c], np.zeros(0, np.int32), np.zeros((0, 4), np.int32))
    assert n.size == 0 and Rt2.shape == (0, 12) and masks == []


def _events(b, limit=None):
    out = []
    while limit is None or len(out) < limit:
        r = b.next()
        if r is None:
            break
        out.append(r)
    return out


def _same_events(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert all(g[k] == w[k] for k in ("cand", "n_inliers", "refined", "no_more")), (g, w)
        assert np.array_equal(g["inliers"], w["inliers"]) and np.array_equal(g["Tcw"].view(np.uint32), w["Tcw"].view(np.uint32))


def test_batch_on_the_device_equals_the_host_evaluator_schedule(ctx):
    from test_pnp_cpu import schedule_fixture
    cands, raws = schedule_fixture()
    sim3.clear_draws()
    h = pnp.PnPRansac(cands, device=None, draws=raws)
    want = _events(h)
    h_stats = h.stats(); h.close()
    assert any(e["refined"] for e in want) and any(e["no_more"] and not e["refined"] for e in want)
    sim3.clear_draws()
    d = pnp.PnPRansac(cands, device=0, draws=raws)
    got = _events(d)
    _same_events(got, want)
    assert d.stats() == h_stats
    d.close()
    sim3.clear_draws()


def test_drop_in_iterate_and_the_fifo_handed_to_a_sim3_batch(ctx):
    """PnPsolver::iterate(5) as shim/PnPsolver_hip.cpp runs it (a single-candidate batch, ccmh_pnp_ransac_iterate) on the device against the host evaluator; then a
    Sim3 batch on the same thread: after the PnP pose it draws from the FIFO what the sequential reference would have drawn next."""
    from ccm_slam_amd import synth
    from test_pnp_cpu import schedule_fixture
    cands, raws = schedule_fixture()
    s3c = [sim3.Sim3Candidate(**d) for d in synth.make_sim3_candidates(70, 1, 1, [25, 20], 0.2)]
    runs = []
    for device in (None, 0):
        sim3.clear_draws()
        b = pnp.PnPRansac(cands[:1], device=device, draws=raws)
        calls = []
        for _ in range(3):
            pose, no_more = b.iterate(0, 5)
            calls.append((pose, no_more, b.info(0)[0], sim3.draws_pending()))
            if no_more:
                break
        src = b.stats()[0]
        s = sim3.Sim3Ransac(s3c, device=0, draws=raws[src:], max_iterations=40)
        ev = s.next()
        runs.append((calls, src, ev, sim3.draws_pending()))
        s.close(); b.close()
    sim3.clear_draws()
    (hc, hs, hev, hleft), (dc, ds, dev, dleft) = runs
    assert hc[0][0] is not None and hc[0][0]["refined"] and hc[0][3].size > 0     # the first call succeeds before its hypotheses run out
    assert len(hc) == len(dc) and hs == ds and np.array_equal(hleft, dleft)
    for (p, nm, its, pend), (q, nm2, its2, pend2) in zip(hc, dc):
        assert nm == nm2 and its == its2 and (p is None) == (q is None) and np.array_equal(pend, pend2)
        if p is not None:
            _same_events([q], [p])
    # the FIFO after the first pose holds the values the sequential solver would have drawn next
    _, _, used = pc.sequential_events(cands[:1], raws, max_events=1)
    assert np.array_equal(hc[0][3], raws[used:used + hc[0][3].size])
    # the Sim3 batch after the host-evaluator PnP and the one after the device PnP saw the same draws: the same event
    assert (hev is None) == (dev is None)
    if hev is not None:
        assert hev[0] == dev[0] and hev[5] == dev[5] and np.array_equal(hev[4], dev[4]) and np.array_equal(hev[1], dev[1])
