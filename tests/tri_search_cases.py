"""Cases shared by tests/test_tri_search_cpu.py and tests/test_tri_search_gpu.py (no test lives here): CreateNewMapPoints' SearchForTriangulation on keyframes of a
keyframe store.

A case is two keyframes (descriptors, undistorted keypoints, octaves, angles, feature vector, map-point flags), F12 and the translation t2 of keyframe 2 (keyframe 1 sits
at the identity pose and keyframe 2 has the identity rotation, so the reference's epipole :708-714 is fx t2x / t2z + cx, fy t2y / t2z + cy in f32: epipole()).
frame_case(frames): the two ORB frames, the feature vectors, F12 and pose of tests/test_ref_matcher.py's SearchForTriangulation test.  planted_cases(): keyframes of
at most 200 features built so that one property each is certain.  install() puts a case's keyframes into a store.

replay() is a literal Python replay of ORBmatcher.cpp:700-852 with CheckDistEpipolarLine (:159-176) and ComputeThreeMaxima (:1607-1648) in numpy f32 with the double
comparison; it shares nothing with csrc/tri_search_math.h and calls nothing of the project.  It also records, per feature of keyframe 1, (status, bestIdx2, bestDist)
before the orientation filter, and the three counters of ccm_tri_search_eval_resident.
"""
import numpy as np

import tests.test_ref_matcher as trm
from ccm_slam_amd import fuse_sim3 as fs, synth

f32 = np.float32
K4 = np.array(synth.EUROC_K, f32)
REC = fs.kf_record(K4, fs.BOUNDS)
SF, S2 = synth.scale_tables()[0], synth.scale_tables()[2]
TH_LOW, HISTO_LENGTH = 50, 30
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
F_ROWS = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], f32)   # a = 0, b = 1, c = -y1: the epipolar line of (x1, y1) is y2 = y1, num = y2 - y1 and den = 1 exactly
T_FAR = np.array([-0.3, 0.0, 0.1], f32)                # the epipole at about (-1009, 248): no keypoint is near it


def hamming(a, b) -> int:
    return int(_POP[np.bitwise_xor(a, b)].sum())


def epipole(t2):
    """:708-714 for Cw = 0, R2w = I: C2 = t2w, in f32 step by step"""
    t2 = np.asarray(t2, f32)
    invz = f32(1.0) / t2[2]
    return f32(f32(f32(K4[0] * t2[0]) * invz) + K4[2]), f32(f32(f32(K4[1] * t2[1]) * invz) + K4[3])


class Kf:
    """one keyframe: descriptors (n, 32), mvKeysUn (x, y, octave, angle), the feature vector (node, off, idx) and the map-point flags"""

    def __init__(self, desc, x, y, octave, angle, fv, has):
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.n = self.desc.shape[0]
        self.x = np.ascontiguousarray(x, f32).reshape(-1); self.y = np.ascontiguousarray(y, f32).reshape(-1)
        self.octave = np.ascontiguousarray(octave, np.int32).reshape(-1)
        self.angle = np.ascontiguousarray(angle, f32).reshape(-1)
        self.fv = tuple(np.ascontiguousarray(v, np.int32) for v in fv)
        self.has = np.ascontiguousarray(has, np.uint8).reshape(-1)
        assert self.x.size == self.y.size == self.octave.size == self.angle.size == self.has.size == self.n


class Case:
    def __init__(self, name, kf1: Kf, kf2: Kf, F12, t2):
        self.name, self.kf1, self.kf2 = name, kf1, kf2
        self.F12 = np.ascontiguousarray(F12, f32).reshape(9)
        self.t2 = np.ascontiguousarray(t2, f32).reshape(3)
        self.ex, self.ey = epipole(self.t2)

    def job(self, key1, key2, has1=None, has2=None):
        return (key1, key2, self.kf1.has if has1 is None else has1, self.kf2.has if has2 is None else has2, self.F12, self.ex, self.ey)


def fv_of(node_of):
    """the flat FeatureVector of a node id per feature (-1: the feature's word is stopped, it is in no node): nodes ascending, indices ascending inside a node"""
    node_of = np.asarray(node_of)
    nodes = np.unique(node_of[node_of >= 0])
    off, idx = [0], []
    for nd in nodes:
        idx.extend(np.flatnonzero(node_of == nd).tolist())
        off.append(len(idx))
    return nodes.astype(np.int32), np.array(off, np.int32), np.array(idx, np.int32)


def add_keyframe(store, key, kf: Kf, featvec=True):
    store.add([key], REC, [0, kf.n], np.stack([kf.x, kf.y], 1), kf.octave.astype(np.uint8), kf.desc)
    if featvec:
        store.set_featvec(key, kf.fv, kf.angle)


def install(store, key1, key2, case: Case):
    add_keyframe(store, key1, case.kf1)
    add_keyframe(store, key2, case.kf2)


def frame_case(frames, seed=3, n_nodes=60, t2=(-0.12, 0.01, 0.02)):
    """tests/test_ref_matcher.py test_search_for_triangulation_M5_with_the_references_own_epipole: its frames, feature vectors, masks, F12 and T2"""
    (k1, d1), (k2, d2) = frames
    rng = np.random.default_rng(seed)
    has1 = (rng.random(len(k1)) < 0.3).astype(np.uint8); has2 = (rng.random(len(k2)) < 0.3).astype(np.uint8)
    t2 = np.array(t2, f32)
    Kk = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1]], np.float64)
    t = -t2.astype(np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F12 = (np.linalg.inv(Kk).T @ tx @ np.linalg.inv(Kk)).astype(f32)
    mk = lambda k, d, has: Kf(d, k["x"], k["y"], k["octave"], k["angle"], trm._feature_vector(d, 0, n_nodes), has)
    return Case(f"frames, {n_nodes} nodes", mk(k1, d1, has1), mk(k2, d2, has2), F12, t2)


def _flip(rng, d, nbits):
    """a copy of descriptor d with nbits distinct bits flipped"""
    bits = np.unpackbits(d)
    bits[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(bits)


def _shuffled_nodes(rng, sizes):
    """node_of for features whose nodes are interleaved: node ids sizes.keys(), sizes.values() features each"""
    node_of = np.concatenate([np.full(s, nd) for nd, s in sizes.items()])
    return rng.permutation(node_of)


class _Side:
    """a keyframe under construction: random descriptors (about 128 bits from anything), every keypoint on the row y = 100 at octave 0, no map points"""

    def __init__(self, rng, sizes):
        self.node = _shuffled_nodes(rng, sizes)
        n = self.n = self.node.size
        assert n <= 200
        self.desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        self.x = rng.uniform(20, 700, n).astype(f32); self.y = np.full(n, 100, f32)
        self.octave = np.zeros(n, np.int32); self.angle = rng.uniform(0, 360, n).astype(f32)
        self.has = np.zeros(n, np.uint8)

    def of(self, node):
        """the features of a node in list order (ascending index)"""
        return np.flatnonzero(self.node == node)

    def kf(self):
        return Kf(self.desc, self.x, self.y, self.octave, self.angle, fv_of(self.node), self.has)


def ulp_numerators(thr: float) -> dict:
    """{"below": (a, b, num), "above": (a, b, num)}: f32 values with den = a * a + b * b exact (small integers) and fl(fl(num * num) / den) equal to the largest f32
    below thr / the smallest f32 not below thr (thr is a double).  num = F12(2, 2) with the candidate at the origin, so num is exact as well."""
    below = f32(thr)
    if float(below) >= thr:
        below = np.nextafter(below, f32(-np.inf))
    above = np.nextafter(below, f32(np.inf))
    assert float(below) < thr <= float(above)
    found = {}
    for a in range(1, 8):
        for b in range(0, 8):
            den = f32(a * a + b * b)
            num = f32(np.sqrt(thr * float(den)))
            for _ in range(40):
                num = np.nextafter(num, f32(-np.inf))
            for _ in range(80):
                dsqr = f32(f32(num * num) / den)
                if dsqr == below:
                    found.setdefault("below", (f32(a), f32(b), num))
                if dsqr == above:
                    found.setdefault("above", (f32(a), f32(b), num))
                num = np.nextafter(num, f32(np.inf))
    assert len(found) == 2, "no exact numerator found"
    return found


def planted_cases():
    out = []
    rng = np.random.default_rng(78)

    def plant_queries(s1, s2, per_query_bits=lambda: int(rng.integers(0, 60))):
        """five in six features of keyframe 1 become a noisy copy of a candidate of their node: 0 .. 59 bits flipped (some beyond TH_LOW), the row shifted by up to
        5 px (some beyond the line gate of the candidate's octave)"""
        for i in range(s1.n):
            c = s2.of(s1.node[i])
            if i % 6 == 0 or s1.node[i] < 0 or c.size == 0:
                continue
            t = int(rng.choice(c))
            s1.desc[i] = _flip(rng, s2.desc[t], per_query_bits())
            s1.y[i] = s2.y[t] + f32(rng.choice([0.0, 0.5, 1.5, 2.5, 5.0]) * rng.choice([-1.0, 1.0]))

    def general(name, sizes1, sizes2):
        s1, s2 = _Side(rng, sizes1), _Side(rng, sizes2)
        s2.y = (np.round(rng.uniform(90, 110, s2.n) * 4) / 4).astype(f32)
        s2.octave = rng.integers(0, 4, s2.n).astype(np.int32)
        plant_queries(s1, s2)
        s1.has = (rng.random(s1.n) < 0.1).astype(np.uint8); s2.has = (rng.random(s2.n) < 0.1).astype(np.uint8)
        out.append(Case(name, s1.kf(), s2.kf(), F_ROWS, T_FAR))

    # keyframe-2 segments of 1, 63, 64, 65, 128 and 129 candidates, 6 queries each (three keyframes of at most 200 features)
    general("segments 1 63 64", {nd: 6 for nd in (10, 11, 12)}, {10: 1, 11: 63, 12: 64})
    general("segments 65 128", {nd: 6 for nd in (13, 14)}, {13: 65, 14: 128})
    general("segment 129", {15: 6}, {15: 129})
    # keyframe-1 nodes of 65 and of 130 queries (two and three chunks of 64)
    general("query nodes of 65 and 130", {3: 65, 4: 130}, {3: 5, 4: 70})
    # keyframe-1 nodes keyframe 2 lacks: before its first (1), between two (25), after its last (40); node 20 is common; stopped-word features (-1) on both sides
    general("absent nodes, stopped words", {1: 5, 20: 12, 25: 4, 40: 6, -1: 9}, {10: 8, 20: 9, 30: 5, -1: 6})

    # ties.  node 7: equal best distances at list positions 63 and 64 (64 wins: the later pass); node 8: the nearer one at 63, a farther one at 64 (63 stays);
    # node 9: equal distances at positions 5 and 11 of one pass (11 wins)
    s1, s2 = _Side(rng, {7: 1, 8: 1, 9: 1}), _Side(rng, {7: 70, 8: 70, 9: 20})
    q7, q8, q9 = int(s1.of(7)[0]), int(s1.of(8)[0]), int(s1.of(9)[0])
    p7, p8, p9 = s2.of(7), s2.of(8), s2.of(9)
    s2.desc[p7[63]] = _flip(rng, s1.desc[q7], 3); s2.desc[p7[64]] = _flip(rng, s1.desc[q7], 3)
    s2.desc[p8[63]] = _flip(rng, s1.desc[q8], 2); s2.desc[p8[64]] = _flip(rng, s1.desc[q8], 3)
    s2.desc[p9[5]] = _flip(rng, s1.desc[q9], 7); s2.desc[p9[11]] = _flip(rng, s1.desc[q9], 7)
    out.append(Case("ties", s1.kf(), s2.kf(), F_ROWS, T_FAR))

    # thresholds and gates, one node each.  31: a candidate at distance 50 (accepted).  32: one at 51 (rejected).  33: the nearest (5) is 10 rows off the line,
    # a farther one (20) is on it.  34: the nearest (4) lies inside the epipole's radius, a farther one (25) outside.  35: two queries whose best is the same idx2.
    t_near = np.array([(300 - K4[2]) / K4[0] * 0.1, (200 - K4[3]) / K4[1] * 0.1, 0.1], f32)   # the epipole at about (300, 200)
    ex, ey = epipole(t_near)
    s1, s2 = _Side(rng, {31: 1, 32: 1, 33: 1, 34: 1, 35: 2}), _Side(rng, {31: 6, 32: 6, 33: 6, 34: 6, 35: 6})
    q = {nd: s1.of(nd) for nd in (31, 32, 33, 34, 35)}
    c = {nd: s2.of(nd) for nd in (31, 32, 33, 34, 35)}
    s2.desc[c[31][2]] = _flip(rng, s1.desc[q[31][0]], 50)
    s2.desc[c[32][2]] = _flip(rng, s1.desc[q[32][0]], 51)
    s2.desc[c[33][1]] = _flip(rng, s1.desc[q[33][0]], 5); s2.y[c[33][1]] = 110
    s2.desc[c[33][4]] = _flip(rng, s1.desc[q[33][0]], 20)
    s1.y[q[34][0]] = ey + f32(4); s2.y[c[34]] = ey + f32(4)
    s2.desc[c[34][0]] = _flip(rng, s1.desc[q[34][0]], 4); s2.x[c[34][0]] = ex + f32(3)       # 3 * 3 + 4 * 4 = 25 < 100 sf[0]
    s2.desc[c[34][3]] = _flip(rng, s1.desc[q[34][0]], 25); s2.x[c[34][3]] = ex + f32(100)
    s2.desc[c[35][3]] = _flip(rng, s1.desc[q[35][0]], 6); s1.desc[q[35][1]] = _flip(rng, s2.desc[c[35][3]], 9)
    out.append(Case("thresholds and gates", s1.kf(), s2.kf(), F_ROWS, t_near))

    # dsqr one f32 ulp below and above 3.84 sigma2, octaves 0 and 2: F12 = [0 0 0; 0 0 0; a b num], every candidate at the origin, so a and b are the line's,
    # num = 0 + 0 + F12(2, 2) and den = a a + b b are exact, and dsqr = fl(fl(num num) / den)
    for o in (0, 2):
        for side, (a, b, num) in sorted(ulp_numerators(3.84 * float(S2[o])).items()):
            s1, s2 = _Side(rng, {2: 3}), _Side(rng, {2: 4})
            s2.x[:] = 0; s2.y[:] = 0; s2.octave[:] = o
            for i in range(3):
                s1.desc[i] = _flip(rng, s2.desc[i], 2 + i)
            out.append(Case(f"dsqr one ulp {side} the threshold, octave {o}", s1.kf(), s2.kf(), [0, 0, 0, 0, 0, 0, a, b, num], T_FAR))

    # a = b = 0: den == 0, CheckDistEpipolarLine returns false for every pair
    s1, s2 = _Side(rng, {2: 3, 6: 2}), _Side(rng, {2: 4, 6: 3})
    for i in range(s1.n):
        s1.desc[i] = _flip(rng, s2.desc[int(s2.of(s1.node[i])[0])], 3)
    out.append(Case("den == 0", s1.kf(), s2.kf(), [0, 0, 0, 0, 0, 0, 0, 0, 1], T_FAR))
    # NaN in F12: b is NaN, every comparison is false, nothing is accepted
    nan_F = F_ROWS.copy(); nan_F[7] = np.nan
    out.append(Case("NaN in F12", s1.kf(), s2.kf(), nan_F, T_FAR))
    # the same keyframes on the plain rows: everything matches (what the two cases above would give without their F12)
    out.append(Case("the den / NaN keyframes on plain rows", s1.kf(), s2.kf(), F_ROWS, T_FAR))

    # node 3: every candidate has a map point (status 1, no distance counted); node 5: every query has one (status 0)
    s1, s2 = _Side(rng, {3: 6, 5: 6}), _Side(rng, {3: 10, 5: 10})
    plant_queries(s1, s2, lambda: 4)
    s2.has[s2.node == 3] = 1; s1.has[s1.node == 5] = 1
    out.append(Case("every candidate with a map point, every query with a map point", s1.kf(), s2.kf(), F_ROWS, T_FAR))
    return out


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


def check_dist_epipolar_line(x1, y1, x2, y2, oct2, F12, sigma2) -> bool:
    """:159-176; F12.at(r, c) = F12[3 r + c]"""
    a = f32(f32(f32(x1 * F12[0]) + f32(y1 * F12[3])) + F12[6])
    b = f32(f32(f32(x1 * F12[1]) + f32(y1 * F12[4])) + F12[7])
    c = f32(f32(f32(x1 * F12[2]) + f32(y1 * F12[5])) + F12[8])
    num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
    den = f32(f32(a * a) + f32(b * b))
    if den == 0:
        return False
    dsqr = f32(f32(num * num) / den)
    return bool(float(dsqr) < 3.84 * float(sigma2[oct2]))


def replay(case: Case, check_orientation, has1=None, has2=None, sf=SF, sigma2=S2):
    """ORBmatcher.cpp:700-852 line by line under the map-point flags has1 / has2 (default: the case's).  Returns nmatches, matches12, words (n1 x 3: status,
    bestIdx2, bestDist before the orientation filter) and (n_query, n_match, n_dist)."""
    k1, k2 = case.kf1, case.kf2
    has1 = k1.has if has1 is None else has1
    has2 = k2.has if has2 is None else has2
    F12, ex, ey = case.F12, case.ex, case.ey
    matches12 = -np.ones(k1.n, np.int32)
    matched2 = np.zeros(k2.n, bool)        # vbMatched2: declared, tested, never set
    words = np.zeros((k1.n, 3), np.int64); words[:, 1] = -1
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    factor = f32(1.0) / f32(HISTO_LENGTH)
    nmatches = n_query = n_match = n_dist = 0
    nodes1, nodes2 = k1.fv[0], k2.fv[0]
    i = j = 0
    with np.errstate(all="ignore"):
        while i < nodes1.size and j < nodes2.size:
            if nodes1[i] == nodes2[j]:
                for idx1 in k1.fv[2][k1.fv[1][i]:k1.fv[1][i + 1]]:
                    if has1[idx1]:
                        continue
                    best_dist, best_idx2 = TH_LOW, -1
                    for idx2 in k2.fv[2][k2.fv[1][j]:k2.fv[1][j + 1]]:
                        if matched2[idx2] or has2[idx2]:
                            continue
                        n_dist += 1
                        dist = hamming(k1.desc[idx1], k2.desc[idx2])
                        if dist > TH_LOW or dist > best_dist:
                            continue
                        distex = f32(ex - k2.x[idx2]); distey = f32(ey - k2.y[idx2])
                        if f32(f32(distex * distex) + f32(distey * distey)) < f32(f32(100) * sf[k2.octave[idx2]]):
                            continue
                        if check_dist_epipolar_line(k1.x[idx1], k1.y[idx1], k2.x[idx2], k2.y[idx2], k2.octave[idx2], F12, sigma2):
                            best_idx2, best_dist = int(idx2), dist
                    n_query += 1
                    words[idx1] = (2 if best_idx2 >= 0 else 1, best_idx2, best_dist)
                    if best_idx2 >= 0:
                        n_match += 1
                        matches12[idx1] = best_idx2
                        nmatches += 1
                        if check_orientation:
                            rot = f32(k1.angle[idx1] - k2.angle[best_idx2])
                            if rot < 0.0:
                                rot = f32(rot + f32(360.0))
                            b = _round_half_away(f32(rot * factor))
                            if b == HISTO_LENGTH:
                                b = 0
                            rot_hist[b].append(int(idx1))
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
    return nmatches, matches12, words, (n_query, n_match, n_dist)


def oracle_call(case: Case, check_orientation, has1=None, has2=None):
    """oracle.search_for_triangulation on the case under the given flags"""
    import oracle
    k1, k2 = case.kf1, case.kf2
    return oracle.search_for_triangulation(k1.fv, k2.fv, k1.has if has1 is None else has1, k2.has if has2 is None else has2, k1.desc, k1.x, k1.y, k1.angle, k2.desc,
                                           k2.x, k2.y, k2.octave, k2.angle, case.F12, float(case.ex), float(case.ey), S2, SF, check_orientation)


def sequence_cases(frames):
    """one new keyframe and six neighbours of the fan-out test of tests/test_ref_matcher.py, each with its own pose, F12 and flags: (cases, has1 of the build)"""
    import oracle
    (k1, d1), _ = frames
    o = oracle.OrbOracle(1000)
    nbs = [o.extract(synth.gen_image(1000 + j // 5, 1 + j % 5)) for j in range(6)]
    o.close()
    out = [frame_case(((k1, d1), nb), seed=21 + j, t2=(-0.12 - 0.01 * j, 0.01 * (j % 3), 0.02)) for j, nb in enumerate(nbs)]
    return out, out[0].kf1.has


def run_sequence(store, seq, has1, host, ori=0):
    """the reference's loop: every call under the flags of its moment; every matched pair becomes a map point of both keyframes before the next call"""
    C6 = len(seq)
    total = 0
    from ccm_slam_amd import tri_search as ts
    with ts.Batch(store, 100, [101 + j for j in range(C6)], has1, [c.kf2.has for c in seq], [(c.F12, c.ex, c.ey) for c in seq], S2, SF, ori, host=host) as b:
        has1_now = has1.copy()
        for j, c in enumerate(seq):
            exp_n, exp = oracle_call(c, ori, has1=has1_now)
            n, m = b.resolve(j, has1_now, None)
            assert n == exp_n and np.array_equal(m, exp), j
            has1_now[exp >= 0] = 1
            total += exp_n
        assert b.reevaluated == 0
        # predicted(j): the flags of the build, as vMatchedPairs
        exp_n, exp = oracle_call(seq[2], ori, has1=has1)
        pairs = b.predicted(2)
        assert pairs.shape == (exp_n, 2) and np.array_equal(pairs[:, 0], np.flatnonzero(exp >= 0)) and np.array_equal(pairs[:, 1], exp[exp >= 0])
        tables = b.tables()
    return total, tables


def install_sequence(store, seq):
    add_keyframe(store, 100, seq[0].kf1)
    for j, c in enumerate(seq):
        add_keyframe(store, 101 + j, c.kf2)


def same_words(got: dict, off, j, case: Case, tag, has1=None, has2=None):
    """job j of a pair_eval result against the replay"""
    from ccm_slam_amd import tri_search as ts
    _, _, words, (n_query, n_match, n_dist) = replay(case, 0, has1, has2)
    table = got["table"][off[j]:off[j + 1]]
    u = ts.unpack(table)
    assert u["status"].size == case.kf1.n, tag
    assert np.array_equal(u["status"], words[:, 0]), tag
    q = words[:, 0] > 0
    assert np.array_equal(u["idx"][q], words[q, 1]) and np.array_equal(u["dist"][q], words[q, 2]), tag
    assert not table[~q].any(), tag
    assert (got["n_query"][j], got["n_match"][j], got["n_dist"][j]) == (n_query, n_match, n_dist), (tag, got["n_query"][j], got["n_match"][j], got["n_dist"][j], n_query,
                                                                                                   n_match, n_dist)


def same_result(got: dict, want: dict, tag):
    assert np.array_equal(got["table"], want["table"]), tag
    for k in ("n_query", "n_match", "n_dist"):
        assert np.array_equal(got[k], want[k]), (tag, k)
