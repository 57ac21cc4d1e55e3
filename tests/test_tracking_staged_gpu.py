"""GPU: the eight host-pointer entry points of a tracked frame and LocalMapping (dense, CSR single and multi, BoW transform, frustum, normal and
depth on staged blocks; window search and distinctive descriptors hand-packed, on the same pinned block) alternate on ONE context through sizes tiny -> mid -> big
-> mid -> tiny, so that the device scratch and the pinned block are regrown between calls and then reused at a smaller size; some calls start right behind a ccm_frame_set_keypoints
and a ccm_pose_optimize call, i.e. on a stream that is still busy.  Every result equals the oracle's (exact, as in test_hamming_gpu.py / test_frame_gpu.py) and
what the same call gives on a fresh context.  The shapes are the smallest at which a layout can go wrong: Q = 1, empty lists, n_cand = 0, T = 0, an odd number of
16-bit distances in front of the int32 outputs, every combination of optional outputs, an empty middle search, list lengths for G = 8 / 32 / wave per query,
several dense splits, a byte segment that is no whole word, a capacity one short of the total."""
import ctypes as C

import numpy as np
import pytest

from test_frame_gpu import _frustum_case
from test_oracle_match import _normal_depth_case

KP = [("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")]


def _fresh(call):
    from ccm_slam_amd._lib import Context
    c = Context(0)
    try:
        return call(c)
    finally:
        c.close()


def _same(got, want, tag):
    assert len(got) == len(want), tag
    for i, (g, w) in enumerate(zip(got, want)):
        if g is None or w is None:
            assert g is None and w is None, (tag, i)
            continue
        g, w = np.ascontiguousarray(g).reshape(-1), np.ascontiguousarray(w).reshape(-1)
        assert g.shape == w.shape and (g.tobytes() == w.tobytes() if g.dtype == w.dtype else np.array_equal(g, w)), (tag, i)


def _desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _lists(rng, lens, T):
    off = np.zeros(len(lens) + 1, np.int32); off[1:] = np.cumsum(lens)
    return off, rng.integers(0, max(T, 1), off[-1]).astype(np.int32)


def _outputs(Q, n_cand, want_dist, want_best):
    dist = np.full(n_cand + 2, 0xBEEF, np.uint16) if want_dist else None     # two canaries behind the distances
    best = [np.full(Q + 1, -77, np.int32) for _ in range(3)] if want_best else [None] * 3
    return dist, best


def _trim(dist, best, Q, n_cand):
    if dist is not None:
        assert (dist[n_cand:] == 0xBEEF).all()
    for b in best:
        assert b is None or b[Q] == -77
    return (None if dist is None else dist[:n_cand],) + tuple(None if b is None else b[:Q] for b in best)


def _csr(ctx, q, t, off, idx, want_dist=True, want_best=True):
    from ccm_slam_amd._lib import _p, check, lib
    Q, n_cand = q.shape[0], int(off[-1])
    dist, best = _outputs(Q, n_cand, want_dist, want_best)
    check(lib().ccm_hamming_csr(ctx.handle, _p(q), Q, _p(t), t.shape[0], _p(off), _p(idx), _p(dist), *map(_p, best)), ctx.handle)
    return _trim(dist, best, Q, n_cand)


def _csr_multi(ctx, qs, ts, offs, idxs, want_dist=True, want_best=True):
    from ccm_slam_amd._lib import _p, check, lib
    S = len(qs)
    q_off = np.zeros(S + 1, np.int32); q_off[1:] = np.cumsum([q.shape[0] for q in qs])
    t_off = np.zeros(S + 1, np.int32); t_off[1:] = np.cumsum([t.shape[0] for t in ts])
    c_base = np.concatenate([[0], np.cumsum([int(o[-1]) for o in offs])])
    off = np.concatenate([[0]] + [o[1:].astype(np.int64) + c_base[s] for s, o in enumerate(offs)]).astype(np.int32)
    q, t, idx = np.concatenate(qs), np.concatenate(ts), np.concatenate(idxs).astype(np.int32)
    Q, n_cand = int(q_off[-1]), int(off[-1])
    dist, best = _outputs(Q, n_cand, want_dist, want_best)
    check(lib().ccm_hamming_csr_multi(ctx.handle, S, _p(q), _p(q_off), _p(t), _p(t_off), _p(off), _p(idx), _p(dist), *map(_p, best)), ctx.handle)
    return _trim(dist, best, Q, n_cand)


def _mask(want, want_dist, want_best):
    return ((want[0] if want_dist else None),) + tuple(w if want_best else None for w in want[1:])


def _window(fg, qs, cap):
    """one ccm_frame_window_search call into buffers of cap + 3 slots; returns rc, off, the two buffers and n_cand"""
    from ccm_slam_amd._lib import _p, lib
    u, v, r, minl, maxl, qd = qs
    Q = u.size
    off = np.full(Q + 1, -5, np.int32); idx = np.full(cap + 3, -7, np.int32); dist = np.full(cap + 3, 9999, np.uint16); n = C.c_int64(-1)
    rc = lib().ccm_frame_window_search(fg._h, Q, _p(u), _p(v), _p(r), _p(minl), _p(maxl), _p(qd), _p(off), _p(idx) if cap else None, _p(dist) if cap else None,
                                       C.c_int64(cap), C.byref(n))
    return rc, off, idx, dist, n.value


@pytest.mark.gpu
def test_eight_tracking_entry_points_alternate_on_one_context(oracle_lib):
    from ccm_slam_amd import matcher, optimizer, synth
    from ccm_slam_amd._lib import Context
    from ccm_slam_amd.frame import FrameGrid, is_in_frustum, update_normal_and_depth
    rng = np.random.default_rng(16)
    kps = np.zeros(1500, dtype=KP)
    kps["x"] = rng.uniform(20, 730, kps.size); kps["y"] = rng.uniform(20, 460, kps.size); kps["octave"] = rng.integers(0, 8, kps.size)
    kdesc = _desc(rng, kps.size)
    pose = synth.make_pose_problem(n=300, seed=3)
    vocab = synth.make_vocabulary(7, 3, seed=3)
    no_dist = np.zeros(4, np.float32)

    def grid(c):
        g = FrameGrid(c, synth.EUROC_K, no_dist, 752, 480)
        g.set_keypoints(kps, kdesc)
        return g

    ctx = Context(0)
    fg = grid(ctx)
    voc = matcher.Vocabulary(ctx, vocab)
    xy, _, _ = fg.get()
    bounds = fg.bounds

    def both(tag, call, want):
        """the call on the shared context against the oracle and against a fresh context"""
        got = call(ctx)
        _same(got, want, f"{tag}: against the oracle")
        _same(got, _fresh(call), f"{tag}: against a fresh context")
        return got

    def csr(tag, Q, T, lens):
        q, t = _desc(rng, Q), _desc(rng, T)
        off, idx = _lists(rng, lens, T)
        want = oracle_lib.hamming_csr(q, t, off, idx)
        for wd, wb in ((True, True), (True, False), (False, True)):      # both, cand_dist only, best* only
            both(f"csr {tag} dist={wd} best={wb}", lambda c: _csr(c, q, t, off, idx, wd, wb), _mask(want, wd, wb))
        return off

    def csr_multi(tag, shapes):
        qs, ts, offs, idxs = [], [], [], []
        for Q, T, lens in shapes:
            o, i = _lists(rng, lens, T)
            qs.append(_desc(rng, Q)); ts.append(_desc(rng, T)); offs.append(o); idxs.append(i)
        parts = [oracle_lib.hamming_csr(q, t, o, i) for q, t, o, i in zip(qs, ts, offs, idxs)]      # search by search
        want = tuple(np.concatenate([p[k] for p in parts]) for k in range(4))
        for wd, wb in ((True, True), (True, False), (False, True)):
            both(f"csr_multi {tag} dist={wd} best={wb}", lambda c: _csr_multi(c, qs, ts, offs, idxs, wd, wb), _mask(want, wd, wb))

    def dense(tag, Q, T):
        q, t = _desc(rng, Q), _desc(rng, T)
        if T:
            t[rng.integers(0, T)] = q[0]                      # a distance of zero, and ties elsewhere are the oracle's to order
        return both(f"dense {tag}", lambda c: matcher.hamming_dense_best2(c, q, t), oracle_lib.hamming_dense_best2(q, t))

    def distinctive(tag, counts):
        off = np.zeros(len(counts) + 1, np.int32); off[1:] = np.cumsum(counts)
        d = _desc(rng, int(off[-1]))
        return both(f"distinctive {tag}", lambda c: (matcher.distinctive_descriptors(c, d, off),), (oracle_lib.distinctive_descriptors(d, off),))

    def bow(tag, N):
        d = _desc(rng, N)
        want = oracle_lib.bow_transform(vocab, d, 2)

        def call(c):
            v = voc if c is ctx else matcher.Vocabulary(c, vocab)
            try:
                return v.transform(d, 2)[:5]
            finally:
                if v is not voc:
                    v.close()
        both(f"bow_transform {tag}", call, want)

    def window(tag, Q, radius):
        at = xy[rng.integers(0, xy.shape[0], Q)] + rng.normal(size=(Q, 2)).astype(np.float32) * 4
        lvl = rng.integers(0, 8, Q).astype(np.int32)
        minl = np.where(rng.random(Q) < 0.3, -1, lvl - 1).astype(np.int32)
        qs = (np.ascontiguousarray(at[:, 0], np.float32), np.ascontiguousarray(at[:, 1], np.float32), np.full(Q, radius, np.float32), minl,
              np.where(minl < 0, -1, lvl).astype(np.int32), _desc(rng, Q))
        off_o, idx_o = oracle_lib.grid_candidates(xy[:, 0], xy[:, 1], kps["octave"], bounds, *qs[:5])
        dist_o = oracle_lib.hamming_csr(qs[5], kdesc, off_o, idx_o)[0]
        total = int(off_o[-1])
        assert total > 2, tag

        def at_cap(cap):
            def call(c):
                g = fg if c is ctx else grid(c)
                try:
                    return _window(g, qs, cap)
                finally:
                    if g is not fg:
                        g.close()
            rc, off, idx, dist, n = call(ctx)
            frc, foff, fidx, fdist, fn = _fresh(call)
            assert (rc, n) == (frc, fn) and n == total, (tag, cap)
            _same((off, idx, dist), (foff, fidx, fdist), f"window {tag} cap {cap}: against a fresh context")
            assert np.array_equal(off, off_o), (tag, cap)           # cand_off and n_cand are filled whatever the capacity
            if cap >= total:
                assert rc == 0 and np.array_equal(idx[:total], idx_o) and np.array_equal(dist[:total], dist_o), (tag, cap)
                assert (idx[total:] == -7).all() and (dist[total:] == 9999).all(), (tag, cap)
            else:                                                   # the sizing call, and a capacity that is too small: nothing is written, canaries included
                assert (rc != 0) == (cap > 0) and (idx == -7).all() and (dist == 9999).all(), (tag, cap)
        at_cap(0)                                   # the sizing call
        at_cap(total)                               # exactly
        at_cap(total + 1 + total % 2)               # odd: the 16-bit distances end on half a word
        at_cap(total - 1)                           # one short
        return total

    def frustum(tag, n):
        frame24, P, normal, dmin, dmax = _frustum_case(4, n)
        return both(f"frustum {tag}", lambda c: is_in_frustum(c, frame24, 8, P, normal, dmin, dmax, 0.5), oracle_lib.is_in_frustum(frame24, 8, P, normal, dmin, dmax, 0.5))

    def normal_depth(tag, k, n_kf=4):
        k = np.asarray(k)
        n_pt = k.size
        pos, _, _, kfc, _, ref_level, sf, old = _normal_depth_case(7, n_pt, n_kf)
        off = np.zeros(n_pt + 1, np.int32); off[1:] = np.cumsum(k)
        obs = np.concatenate([rng.permutation(n_kf)[:kk] for kk in k] + [np.zeros(0, np.int64)]).astype(np.int32)
        ref_kf = np.array([obs[off[i]] if k[i] else 0 for i in range(n_pt)], np.int32)
        args = (pos, off, obs, kfc, ref_kf, ref_level, sf) + tuple(old)
        got = both(f"normal_and_depth {tag}", lambda c: update_normal_and_depth(c, *args), oracle_lib.update_normal_and_depth(*args))
        for i in np.nonzero(k == 0)[0]:                             # a point without observers keeps the seeded values
            assert all(np.array_equal(g[i], o[i]) for g, o in zip(got, old)), (tag, i)
        return got

    def busy():
        """leaves the stream with work in flight: the keypoint upload and grid build of the frame (the same keypoints: what the windows search stays what the
        oracle was given), then a pose optimisation"""
        fg.set_keypoints(kps, kdesc)
        optimizer.pose_optimization(ctx, pose["cam_qt"], pose["Xw"], pose["obs"], pose["info"], pose["K"])

    def tiny(tag):
        csr(f"{tag}: Q = 1, one candidate", 1, 1, [1])
        dense(f"{tag}: 1 x 1", 1, 1)
        csr_multi(f"{tag}: one search of one query", [(1, 1, [1])])
        assert distinctive(f"{tag}: P = 1, one observation", [1])[0][0] == 0
        bow(f"{tag}: N = 1", 1)
        window(f"{tag}: Q = 1", 1, 60.0)
        frustum(f"{tag}: n = 1", 1)
        normal_depth(f"{tag}: n_pt = 1", [2])
        csr(f"{tag}: an empty list, odd n_cand", 3, 5, [2, 0, 3])
        assert (dense(f"{tag}: T = 0", 3, 0)[0] == -1).all()
        csr(f"{tag}: n_cand = 0", 2, 4, [0, 0])
        assert distinctive(f"{tag}: a point without observations", [2, 0, 3])[0][1] == -1
        csr(f"{tag}: T = 0", 2, 0, [0, 0])
        assert (distinctive(f"{tag}: total = 0", [0, 0])[0] == -1).all()
        bow(f"{tag}: N = 5", 5)
        frustum(f"{tag}: n = 7", 7)
        normal_depth(f"{tag}: n_obs = 0", [0, 0, 0])
        normal_depth(f"{tag}: one point without observers", [3, 1, 0, 2, 4])
        csr_multi(f"{tag}: S = 3, the middle search empty", [(2, 3, [1, 2]), (0, 2, []), (3, 4, [0, 3, 1])])

    def mid(tag):
        busy()
        off = csr(f"{tag}: G = 8, behind a busy stream", 200, 150, rng.poisson(5, 200))
        assert off[-1] / 200 <= 16
        dense(f"{tag}: 65 x 130, several splits", 65, 130)
        csr_multi(f"{tag}: S = 4", [(60, 80, rng.poisson(20, 60)), (0, 10, []), (45, 70, rng.poisson(9, 45)), (30, 20, np.zeros(30, np.int64))])
        busy()
        window(f"{tag}: Q = 120, behind a busy stream", 120, 25.0)
        distinctive(f"{tag}: 300 points", rng.integers(0, 40, 300))
        off = csr(f"{tag}: G = 32", 150, 300, 33 + rng.poisson(12, 150))
        assert 32 < off[-1] / 150 <= 64
        frustum(f"{tag}: n = 3001", 3001)
        bow(f"{tag}: N = 700", 700)
        busy()
        normal_depth(f"{tag}: 2000 points, behind a busy stream", np.clip(rng.poisson(4, 2000), 0, 30), n_kf=40)

    try:
        tiny("first, on an empty scratch")
        mid("growing")
        # big: every buffer is regrown once more; the dense call stands between two larger staged calls
        off = csr("big: a wave per query", 400, 900, 70 + rng.poisson(25, 400))
        assert off[-1] / 400 > 64
        dense("big: 65 x 130 between two larger calls", 65, 130)
        busy()
        dense("big: 1500 x 2000, behind a busy stream", 1500, 2000)
        window("big: Q = 1500", 1500, 40.0)
        frustum("big: n = 20000", 20000)
        mid("shrinking")
        tiny("again, in the grown buffers")
    finally:
        voc.close()
        fg.close()
        ctx.close()
