"""Cases shared by tests/test_bow_search_cpu.py and tests/test_bow_search_gpu.py (no test lives here): ComputeSim3's SearchByBoW on keyframes of a keyframe store
(DESIGN.md §23).

A case is two keyframes (descriptors, angles, feature vector) and their live masks.  frame_case(frames, n_nodes): the two ORB frames of tests/test_ref_matcher.py
with its _feature_vector at n_nodes = 60 (about 17 features per node) or 6 (about 170: more than two passes of 64 candidates, many claims per node).
planted_cases(): small keyframes built so that one property each is certain.  install() puts a case's keyframes into a store.

replay() is a literal Python replay of ORBmatcher.cpp:565-698 (with ComputeThreeMaxima, :1607-1648); it shares nothing with csrc/bow_search_math.h.  It also records,
per query, the reduction on the INITIAL vbMatched2 (what the device evaluates) and whether the claims changed the query's answer.  expected_reeval() counts
independently which queries cslam::SearchByBoWBatch's rule must evaluate again.
"""
import numpy as np

import tests.test_ref_matcher as trm
from ccm_slam_amd import fuse_sim3 as fs, synth

f32 = np.float32
REC = fs.kf_record(np.array(synth.EUROC_K, f32), fs.BOUNDS)
TH_LOW, HISTO_LENGTH = 50, 30
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b) -> int:
    return int(_POP[np.bitwise_xor(a, b)].sum())


class Kf:
    """one keyframe: descriptors (n, 32), angles, the feature vector (node, off, idx) and the live mask"""

    def __init__(self, desc, angle, fv, live):
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.n = self.desc.shape[0]
        self.angle = np.ascontiguousarray(angle, f32).reshape(-1)
        self.fv = tuple(np.ascontiguousarray(x, np.int32) for x in fv)
        self.live = np.ascontiguousarray(live, np.uint8).reshape(-1)
        assert self.angle.size == self.n and self.live.size == self.n


class Case:
    def __init__(self, name, kf1: Kf, kf2: Kf):
        self.name, self.kf1, self.kf2 = name, kf1, kf2


def fv_of(node_of):
    """the flat FeatureVector of a node id per feature (-1: the feature's word is stopped, it is in no node): nodes ascending, indices ascending inside a node"""
    node_of = np.asarray(node_of)
    nodes = np.unique(node_of[node_of >= 0])
    off, idx = [0], []
    for nd in nodes:
        idx.extend(np.flatnonzero(node_of == nd).tolist())
        off.append(len(idx))
    return nodes.astype(np.int32), np.array(off, np.int32), np.array(idx, np.int32)


def add_keyframe(store, key, kf: Kf, featvec=True, seed=0):
    rng = np.random.default_rng(seed)
    xy = np.stack([rng.uniform(0, 752, kf.n), rng.uniform(0, 480, kf.n)], 1).astype(f32)
    store.add([key], REC, [0, kf.n], xy, np.zeros(kf.n, np.uint8), kf.desc)
    if featvec:
        store.set_featvec(key, kf.fv, kf.angle)


def install(store, key1, key2, case: Case):
    add_keyframe(store, key1, case.kf1, seed=1)
    add_keyframe(store, key2, case.kf2, seed=2)


def frame_case(frames, n_nodes, seed=2):
    (k1, d1), (k2, d2) = frames
    rng = np.random.default_rng(seed)
    has1 = (rng.random(len(k1)) < 0.8).astype(np.uint8); has2 = (rng.random(len(k2)) < 0.8).astype(np.uint8)
    return Case(f"frames, {n_nodes} nodes", Kf(d1, k1["angle"], trm._feature_vector(d1, 0, n_nodes), has1), Kf(d2, k2["angle"], trm._feature_vector(d2, 0, n_nodes), has2))


def _flip(rng, d, nbits):
    """a copy of descriptor d with nbits distinct bits flipped"""
    bits = np.unpackbits(d)
    bits[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(bits)


def _shuffled_nodes(rng, sizes):
    """node_of for features whose nodes are interleaved: node ids sizes.keys(), sizes.values() features each"""
    node_of = np.concatenate([np.full(s, nd) for nd, s in sizes.items()])
    return rng.permutation(node_of)


def planted_cases():
    out = []
    rng = np.random.default_rng(77)
    rnd = lambda n: rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ang = lambda n: rng.uniform(0, 360, n).astype(f32)

    # side-2 segments of 1, 63, 64, 65, 128 and 129 candidates (nodes 10 .. 15), 6 queries each, most of them a few bits from a candidate of their node
    sizes2 = dict(zip(range(10, 16), (1, 63, 64, 65, 128, 129)))
    n2 = _shuffled_nodes(rng, sizes2); d2 = rnd(n2.size)
    n1 = _shuffled_nodes(rng, {nd: 6 for nd in sizes2}); d1 = rnd(n1.size)
    for i in range(n1.size):
        if i % 6:
            d1[i] = _flip(rng, d2[rng.choice(np.flatnonzero(n2 == n1[i]))], int(rng.integers(0, 30)))
    out.append(Case("segments 1 63 64 65 128 129", Kf(d1, ang(n1.size), fv_of(n1), rng.random(n1.size) < 0.9), Kf(d2, ang(n2.size), fv_of(n2), rng.random(n2.size) < 0.85)))

    # keyframe-1 nodes keyframe 2 lacks: before its first (1), between two (25), after its last (40); node 20 is common.  Node 30: a single live candidate
    # (bestDist2 = 256, the ratio test passes).  Node 35: every candidate masked (status 1).  Stopped-word features (-1) on both sides.
    n1 = _shuffled_nodes(rng, {1: 5, 20: 7, 25: 4, 30: 3, 35: 3, 40: 6, -1: 9})
    n2 = _shuffled_nodes(rng, {10: 8, 20: 9, 30: 5, 35: 4, -1: 6})
    d1, d2 = rnd(n1.size), rnd(n2.size)
    l1 = np.ones(n1.size, np.uint8); l2 = np.ones(n2.size, np.uint8)
    c30 = np.flatnonzero(n2 == 30); l2[c30[1:]] = 0; l2[n2 == 35] = 0
    for i in np.flatnonzero(n1 == 30):
        d1[i] = _flip(rng, d2[c30[0]], 4 + int(i) % 3)
    for i in np.flatnonzero(n1 == 20)[:4]:
        d1[i] = _flip(rng, d2[rng.choice(np.flatnonzero(n2 == 20))], 9)
    l1[np.flatnonzero(n1 == 20)[-1]] = 0
    out.append(Case("absent nodes, single candidate, all candidates masked, stopped words", Kf(d1, ang(n1.size), fv_of(n1), l1), Kf(d2, ang(n2.size), fv_of(n2), l2)))

    # all descriptors equal: the first index wins, bestDist2 == bestDist1 == 0; 70 candidates (two passes) and one node of 3
    n1 = _shuffled_nodes(rng, {4: 5, 9: 2}); n2 = _shuffled_nodes(rng, {4: 70, 9: 3})
    out.append(Case("all descriptors equal", Kf(np.full((n1.size, 32), 0x5A, np.uint8), ang(n1.size), fv_of(n1), np.ones(n1.size)),
                    Kf(np.full((n2.size, 32), 0x5A, np.uint8), ang(n2.size), fv_of(n2), np.ones(n2.size))))

    # equal best distances at list positions 63 and 64 (node 7: position 63 must win, bestDist2 equal), and the reverse (node 8: best at 64, second at 63)
    n2 = _shuffled_nodes(rng, {7: 130, 8: 130}); d2 = rnd(n2.size)
    n1 = np.array([7, 8, 7, 8]); d1 = rnd(4)
    p7, p8 = np.flatnonzero(n2 == 7), np.flatnonzero(n2 == 8)       # list order = ascending index
    d2[p7[63]] = _flip(rng, d1[0], 3); d2[p7[64]] = _flip(rng, d1[0], 3)
    d2[p8[64]] = _flip(rng, d1[1], 2); d2[p8[63]] = _flip(rng, d1[1], 3)
    out.append(Case("ties across the pass boundary", Kf(d1, ang(4), fv_of(n1), np.ones(4)), Kf(d2, ang(n2.size), fv_of(n2), np.ones(n2.size))))

    # every query masked
    n1 = _shuffled_nodes(rng, {3: 6, 5: 6}); n2 = _shuffled_nodes(rng, {3: 10, 5: 10})
    out.append(Case("every query masked", Kf(rnd(12), ang(12), fv_of(n1), np.zeros(12)), Kf(rnd(20), ang(20), fv_of(n2), np.ones(20))))
    return out


def reduce_initial(case: Case):
    """per feature of keyframe 1: (status, bestDist1, bestIdx2, bestDist2, node2) of :609-639 on the initial vbMatched2, and n_query, n_dist"""
    k1, k2 = case.kf1, case.kf2
    words = np.zeros((k1.n, 5), np.int64)
    pos2 = {int(nd): b for b, nd in enumerate(k2.fv[0])}
    n_query = n_dist = 0
    for a, nd in enumerate(k1.fv[0]):
        if int(nd) not in pos2:
            continue
        b = pos2[int(nd)]
        for idx1 in k1.fv[2][k1.fv[1][a]:k1.fv[1][a + 1]]:
            if not k1.live[idx1]:
                continue
            best1, bidx, best2, cnt = 256, -1, 256, 0
            for idx2 in k2.fv[2][k2.fv[1][b]:k2.fv[1][b + 1]]:
                if not k2.live[idx2]:
                    continue
                cnt += 1
                dist = hamming(k1.desc[idx1], k2.desc[idx2])
                if dist < best1:
                    best2, best1, bidx = best1, dist, int(idx2)
                elif dist < best2:
                    best2 = dist
            words[idx1] = (2 if cnt else 1, best1, bidx, best2, b)
            n_query += 1; n_dist += cnt
    return words, n_query, n_dist


def _three_maxima(histo):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i in range(HISTO_LENGTH):
        s = len(histo[i])
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif max3 < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def _round_half_away(t) -> int:
    t = float(t)
    return int(np.floor(t + 0.5)) if t >= 0 else int(np.ceil(t - 0.5))


def replay(case: Case, nnratio, check_orientation):
    """ORBmatcher.cpp:565-698 line by line: (nmatches, matches12, changed) where changed counts the queries whose (bestDist1, bestIdx2, bestDist2) under the claims
    differs from the reduction on the initial vbMatched2"""
    k1, k2 = case.kf1, case.kf2
    matches12 = -np.ones(k1.n, np.int32)
    matched2 = np.zeros(k2.n, bool)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    factor = f32(1.0) / f32(HISTO_LENGTH)
    nmatches = changed = 0
    initial = reduce_initial(case)[0]
    nodes1, nodes2 = k1.fv[0], k2.fv[0]
    i = j = 0
    while i < nodes1.size and j < nodes2.size:
        if nodes1[i] == nodes2[j]:
            for idx1 in k1.fv[2][k1.fv[1][i]:k1.fv[1][i + 1]]:
                if not k1.live[idx1]:
                    continue
                best1, bidx, best2 = 256, -1, 256
                for idx2 in k2.fv[2][k2.fv[1][j]:k2.fv[1][j + 1]]:
                    if matched2[idx2] or not k2.live[idx2]:
                        continue
                    dist = hamming(k1.desc[idx1], k2.desc[idx2])
                    if dist < best1:
                        best2, best1, bidx = best1, dist, int(idx2)
                    elif dist < best2:
                        best2 = dist
                changed += tuple(initial[idx1][1:4]) != (best1, bidx, best2)
                if best1 < TH_LOW and f32(best1) < f32(nnratio) * f32(best2):
                    matches12[idx1] = bidx
                    matched2[bidx] = True
                    if check_orientation:
                        rot = f32(k1.angle[idx1] - k2.angle[bidx])
                        if rot < 0.0:
                            rot = f32(rot + f32(360.0))
                        b = _round_half_away(f32(rot * factor))
                        if b == HISTO_LENGTH:
                            b = 0
                        rot_hist[b].append(int(idx1))
                    nmatches += 1
            i += 1; j += 1
        elif nodes1[i] < nodes2[j]:
            i = int(np.searchsorted(nodes1, nodes2[j]))
        else:
            j = int(np.searchsorted(nodes2, nodes1[i]))
    if check_orientation:
        keep = _three_maxima(rot_hist)
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for idx1 in rot_hist[b]:
                matches12[idx1] = -1
                nmatches -= 1
    return nmatches, matches12, changed


def expected_reeval(case: Case, nnratio) -> int:
    """the queries the rule of cslam::SearchByBoWBatch evaluates again: evaluated on the device, bestDist1 < TH_LOW, and a feature claimed so far by an earlier query
    of the same node at a distance <= the initial bestDist2.  (The rotation histogram removes matches afterwards and claims nothing back.)"""
    k1, k2 = case.kf1, case.kf2
    initial = reduce_initial(case)[0]
    pos2 = {int(nd): b for b, nd in enumerate(k2.fv[0])}
    count = 0
    for a, nd in enumerate(k1.fv[0]):
        if int(nd) not in pos2:
            continue
        b = pos2[int(nd)]
        seg2 = [int(x) for x in k2.fv[2][k2.fv[1][b]:k2.fv[1][b + 1]]]
        claimed = []
        for idx1 in k1.fv[2][k1.fv[1][a]:k1.fv[1][a + 1]]:
            status, best1, bidx, best2, _ = (int(x) for x in initial[idx1])
            if status != 2 or best1 >= TH_LOW:
                continue
            if any(hamming(k1.desc[idx1], k2.desc[c]) <= best2 for c in claimed):
                count += 1
                best1, bidx, best2 = 256, -1, 256
                for idx2 in seg2:
                    if idx2 in claimed or not k2.live[idx2]:
                        continue
                    dist = hamming(k1.desc[idx1], k2.desc[idx2])
                    if dist < best1:
                        best2, best1, bidx = best1, dist, idx2
                    elif dist < best2:
                        best2 = dist
            if best1 < TH_LOW and f32(best1) < f32(nnratio) * f32(best2):
                claimed.append(bidx)
    return count


def same_words(got: dict, off, j, case: Case, tag):
    """job j of a pair_eval result against reduce_initial(case)"""
    from ccm_slam_amd import bow_search as bs
    words, n_query, n_dist = reduce_initial(case)
    u = bs.unpack(got["table"][off[j]:off[j + 1]])
    assert u["status"].size == case.kf1.n, tag
    assert np.array_equal(u["status"], words[:, 0]), tag
    q = words[:, 0] > 0
    for name, col in (("d1", 1), ("idx", 2), ("d2", 3), ("node2", 4)):
        assert np.array_equal(u[name][q], words[q, col]), (tag, name)
    assert not got["table"][off[j]:off[j + 1]][~q].any(), tag
    assert got["n_query"][j] == n_query and got["n_dist"][j] == n_dist, (tag, got["n_query"][j], n_query, got["n_dist"][j], n_dist)


def same_result(got: dict, want: dict, tag):
    assert np.array_equal(got["table"], want["table"]), tag
    assert np.array_equal(got["n_query"], want["n_query"]) and np.array_equal(got["n_dist"], want["n_dist"]), tag
