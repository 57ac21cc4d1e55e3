"""GPU: ccm_triangulate_pairs (csrc/triangulate.hip) against the numpy checker of tests/test_triangulate_cpu.py — equal status, bit-identical x3D, no
tolerance: every operation is an IEEE add, multiply, divide or square root in f32 or f64 — and cslam::NewMapPointBatch on the device against the
per-neighbour sequence, alone and chained behind TriangulationBatch.resolve."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from test_triangulate_cpu import check_batch, planted_scenes, ref_pairs, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _compare(ctx, args, name=""):
    from ccm_slam_amd import triangulate as T
    st, x3d, nacc = T.triangulate_pairs(ctx, *args)
    rst, rx = ref_pairs(*args)
    bad = np.nonzero(st != rst)[0]
    assert bad.size == 0, (name, bad[:10], st[bad[:10]], rst[bad[:10]])
    assert same_bits(x3d, rx), name
    off = np.asarray(args[2])
    assert list(nacc) == [int((rst[off[s]:off[s + 1]] == 0).sum()) for s in range(off.size - 1)], name
    return st


@pytest.mark.gpu
def test_device_matches_the_checker(ctx):
    from ccm_slam_amd import triangulate as T
    hist = np.zeros(9, np.int64)
    octaves = set()
    for S in range(1, 21):                                           # 1 .. 20 neighbours, some of them without a match
        counts = [(53 * (S + s)) % 90 + 1 for s in range(S)]
        sc = T.make_pair_scene(seed=200 + S, S=S, n_pairs=counts, empty=() if S < 3 else (1, S - 1))
        hist += np.bincount(_compare(ctx, T.flat(sc), f"S = {S}"), minlength=9)
        octaves |= set(sc["oct"].reshape(-1).tolist())
    sc = T.make_pair_scene(seed=230, S=1, n_pairs=1, mismatch=0, behind=0, tiny_baseline=0, wild_octave=0)           # one match
    hist += np.bincount(_compare(ctx, T.flat(sc), "one match"), minlength=9)
    sc = T.make_pair_scene(seed=231, S=20, n_pairs=400)                                                              # 8000 matches
    assert sc["pair_off"][-1] == 8000
    hist += np.bincount(_compare(ctx, T.flat(sc), "8000 matches"), minlength=9)
    sc = T.make_pair_scene(seed=232, S=2, n_pairs=30)
    sc["cam2"][1, 9] = np.nan                                        # a NaN translation goes through the SVD, a NaN keypoint stops at the parallax gate
    sc["xy"][3, 0] = np.nan
    hist += np.bincount(_compare(ctx, T.flat(sc), "nan"), minlength=9)
    for name, args in planted_scenes():
        hist += np.bincount(_compare(ctx, args, name), minlength=9)
    print("status histogram:", dict(zip(T.STATUS, hist.tolist())))
    assert octaves == set(range(8))
    assert (hist > 0).all(), hist                                    # every gate of the reference was reached on the device
    assert hist[0] > 5000 and hist[1] > 300 and hist[8] > 50


@pytest.mark.gpu
def test_planted_cases(ctx):
    """cos exactly 0.9998f and its two neighbours, z = 0, w = 0, a zero distance, 5.991 sigma2 one ulp to either side of a match's squared error."""
    from ccm_slam_amd import triangulate as T
    got = {}
    for name, args in planted_scenes():
        st, x3d, _ = T.triangulate_pairs(ctx, *args)
        rst, rx = ref_pairs(*args)
        assert np.array_equal(st, rst) and same_bits(x3d, rx), name
        got[name] = (st, x3d)
    st, x = got["parallax"]
    assert st[0] != 1 and st[1] == 1 and st[2] == 1 and np.isnan(x[1:]).all() and not np.isnan(x[0]).any()
    assert list(got["z = 0"][0]) == [3] and np.array_equal(got["z = 0"][1][0], np.zeros(3, f32))
    assert list(got["w = 0"][0]) == [2]
    assert list(got["dist1 = 0"][0]) == [7] and list(got["dist2 = 0"][0]) == [7]
    assert got["reprojection 1"][0][0] == 5 and got["reprojection 1"][0][2] == 0
    assert got["reprojection 2"][0][0] == 6 and got["reprojection 2"][0][2] == 0


@pytest.mark.gpu
def test_error_paths(ctx):
    from ccm_slam_amd import triangulate as T
    from ccm_slam_amd._lib import CcmError, lib
    sc = T.make_pair_scene(seed=240, S=3, n_pairs=10)
    args = list(T.flat(sc))
    T.triangulate_pairs(ctx, *args)
    bad = list(args); bad[2] = np.array([0, 20, 10, 30], np.int32)                                   # pair_off decreases
    with pytest.raises(CcmError):
        T.triangulate_pairs(ctx, *bad)
    for v in (-1, 8):                                                                                # an octave outside [0, nlevels)
        bad = list(args); bad[4] = sc["oct"].copy(); bad[4][7, 1] = v
        with pytest.raises(CcmError):
            T.triangulate_pairs(ctx, *bad)
    with pytest.raises(CcmError):                                                                    # S < 1
        T.triangulate_pairs(ctx, sc["cam1"], np.zeros(0, f32), np.zeros(1, np.int32), np.zeros(0, f32), np.zeros(0, np.int32), *args[5:])
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
    keep = [np.ascontiguousarray(a) for a in args[:9]]
    st = np.zeros(30, np.uint8); x = np.zeros(90, f32); na = np.zeros(3, np.int32)
    full = [p(keep[0]), 3, p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), 8, p(keep[5]), p(keep[6]), p(keep[7]), p(keep[8]), C.c_float(1.8), p(st), p(x), p(na)]
    assert lib().ccm_triangulate_pairs(ctx.handle, *full) == 0
    for i in (0, 2, 3, 4, 5, 7, 8, 9, 10, 12, 13, 14):                                               # each pointer in turn
        a = list(full); a[i] = None
        assert lib().ccm_triangulate_pairs(ctx.handle, *a) == -1, i
    assert lib().ccm_triangulate_pairs(None, *full) == -1
    # no match at all: success, no launch, the counts zeroed
    na[:] = 5
    zero = np.zeros(4, np.int32)
    a = list(full); a[3] = p(zero); a[4] = a[5] = a[12] = a[13] = None
    assert lib().ccm_triangulate_pairs(ctx.handle, *a) == 0 and list(na) == [0, 0, 0]


@pytest.mark.gpu
def test_two_threads_with_their_own_contexts_and_a_rerun():
    from ccm_slam_amd import triangulate as T
    from ccm_slam_amd._lib import Context
    scenes = [T.make_pair_scene(seed=250 + i, S=12, n_pairs=150) for i in range(2)]
    want = [ref_pairs(*T.flat(sc)) for sc in scenes]
    out = [None, None]
    err = []

    def worker(i):
        try:
            c = Context(0)
            runs = [T.triangulate_pairs(c, *T.flat(scenes[i])) for _ in range(6)]
            c.close()
            out[i] = runs
        except Exception as e:   # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for i in range(2):
        for st, x3d, _ in out[i]:                                    # every run, the first included, is the checker's answer bit for bit: a re-run is identical
            assert np.array_equal(st, want[i][0]) and same_bits(x3d, want[i][1])
            assert np.array_equal(x3d.view(np.uint32), out[i][0][1].view(np.uint32))


@pytest.mark.gpu
def test_batch_on_the_device_equals_the_per_neighbour_sequence(ctx):
    from ccm_slam_amd import triangulate as T
    misses_seen = 0
    for seed in (0, 1, 2):
        predicted, hits, misses, accepted = check_batch(T.make_keyframe_scene(seed=seed, S=20 if seed == 0 else 8, n_feat=300), 0)
        assert accepted > 100 and hits > 100
        misses_seen += misses
    assert misses_seen > 0
    predicted, hits, misses, accepted = check_batch(T.make_keyframe_scene(seed=5, S=8, n_feat=300, disjoint=True), 0)
    assert misses == 0 and hits == predicted
    # the per-neighbour device calls give the same answers as the batch's table
    sc = T.make_keyframe_scene(seed=7, S=6, n_feat=200)
    has1 = np.zeros(200, np.uint8)
    pred = [T.resolve_candidates(c, has1) for c in sc["cands"]]
    b = T.NewMapPoints(0, sc["cam1"], sc["keys1"], sc["cam2"], sc["keys2"], pred, sc["sigma2"], sc["sf"], sc["sigma2"], sc["sf"], sc["ratio"])
    for j in range(6):
        xy, oct_ = T.pairs_to_flat(sc, j, pred[j])
        st, x3d, _ = T.triangulate_pairs(ctx, sc["cam1"], sc["cam2"][j:j + 1], [0, len(pred[j])], xy, oct_, sc["sigma2"], sc["sf"], sc["sigma2"], sc["sf"], sc["ratio"])
        bst, bx, _ = b.points(j, pred[j])
        assert np.array_equal(st, bst) and same_bits(x3d, bx)
    assert b.stats() == (sum(len(p) for p in pred),) * 2 + (0,)
    b.close()


@pytest.mark.gpu
def test_chain_behind_the_triangulation_batch(ctx):
    """TriangulationBatch.resolve -> NewMapPointBatch.points on synthetic keyframes (descriptors, one vocabulary node, F12 from the poses) against the checker
    chained the same way: resolve neighbour j with the flags as they are, triangulate its matches, an accepted match gives idx1 a map point."""
    from ccm_slam_amd import triangulate as T
    host = C.CDLL(os.path.join(ROOT, "ccm_slam_amd", "libccm_host.so"))
    host.ccmh_tri_batch_create.restype = C.c_void_p
    host.ccmh_tri_batch_destroy.argtypes = [C.c_void_p]
    host.ccmh_tri_batch_destroy.restype = None
    host.ccmh_tri_batch_resolve.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_float, C.c_float] + [C.c_void_p] * 3
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    c = np.ascontiguousarray
    S, N1 = 10, 300
    sc = T.make_keyframe_scene(seed=11, S=S, n_feat=N1, rival=0.0)
    rng = np.random.default_rng(11)
    d1 = rng.integers(0, 256, (N1, 32), dtype=np.uint8)
    d2 = []
    for j in range(S):
        d = rng.integers(0, 256, (sc["keys2"][j][0].size, 32), dtype=np.uint8)
        tr = sc["truth"][j]
        d[tr[:, 1]] = d1[tr[:, 0]]
        flip = rng.integers(0, 256, (len(tr), 3))                     # three flipped bits per true match
        for k in range(3):
            d[tr[:, 1], flip[:, k] // 8] ^= (1 << (flip[:, k] % 8)).astype(np.uint8)
        d2.append(c(d))
    one_node = lambda n: (np.zeros(1, np.int32), np.array([0, n], np.int32), np.arange(n, dtype=np.int32))
    fv1 = one_node(N1); fv2 = [one_node(k[0].size) for k in sc["keys2"]]
    has1 = np.zeros(N1, np.uint8); has2 = [np.zeros(k[0].size, np.uint8) for k in sc["keys2"]]
    a1 = np.zeros(N1, f32); a2 = [np.zeros(k[0].size, f32) for k in sc["keys2"]]
    keep = []

    def ptrs(arrs):
        arrs = [c(a) for a in arrs]
        keep.extend(arrs)
        return (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    nn2 = np.ones(S, np.int32); N2 = np.array([k[0].size for k in sc["keys2"]], np.int32)
    x1, y1, o1 = sc["keys1"]
    h = host.ccmh_tri_batch_create(0, C.c_float(0.6), 0, p(fv1[0]), p(fv1[1]), p(fv1[2]), 1, p(has1), p(d1), p(x1), p(y1), p(a1), N1, S,
                                   ptrs([f[0] for f in fv2]), ptrs([f[1] for f in fv2]), ptrs([f[2] for f in fv2]), p(nn2), ptrs(has2), ptrs(d2),
                                   ptrs([k[0] for k in sc["keys2"]]), ptrs([k[1] for k in sc["keys2"]]), ptrs([k[2] for k in sc["keys2"]]), ptrs(a2), p(N2))
    assert h, "ccmh_tri_batch_create failed"
    Fs, es = zip(*[T.fundamental(sc["cam1"], sc["cam2"][j]) for j in range(S)])
    F12 = c(np.stack(Fs)); exy = c(np.array(es, f32))
    b = T.NewMapPoints.from_tri_batch(0, h, o1, sc["cam1"], sc["cam2"], F12, exy, sc["sigma2"], sc["sf"], sc["sigma2"], sc["sf"], sc["ratio"])
    has1_now = has1.copy()
    total = accepted = 0
    for j in range(S):
        m12 = np.zeros(N1, np.int32)
        n = host.ccmh_tri_batch_resolve(h, j, p(has1_now), p(has2[j]), p(F12[j]), C.c_float(exy[j, 0]), C.c_float(exy[j, 1]), p(sc["sigma2"]), p(sc["sf"]), p(m12))
        i1 = np.nonzero(m12 >= 0)[0]
        pairs = np.stack([i1, m12[i1]], 1).astype(np.int32)
        assert n == len(pairs)
        st, x3d, n_ok = b.points(j, pairs)
        xy, oct_ = T.pairs_to_flat(sc, j, pairs)
        rst, rx = ref_pairs(sc["cam1"], sc["cam2"][j:j + 1], [0, len(pairs)], xy, oct_, sc["sigma2"], sc["sf"], sc["sigma2"], sc["sf"], sc["ratio"])
        assert np.array_equal(st, rst) and same_bits(x3d, rx) and n_ok == int((rst == 0).sum()), j
        has1_now[pairs[st == 0, 0]] = 1
        total += len(pairs); accepted += n_ok
    predicted, hits, misses = b.stats()
    # a feature of keyframe 1 is accepted at most once (it has a map point afterwards), so at most N1 = 300 matches are accepted in the whole chain;
    # nearly every feature is seen by some neighbour (share 0.6 each, ten neighbours) and its true match triangulates
    assert total >= accepted > 200, (total, accepted)
    # SearchForTriangulation never claims a feature of keyframe 2, so a map point gained by keyframe 1 can only REMOVE matches: the prediction covers all of them
    assert misses == 0 and hits == total and predicted > total
    b.close()
    host.ccmh_tri_batch_destroy(h)
