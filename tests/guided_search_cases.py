"""ORBmatcher::SearchByProjection(Frame&, kfptr, const set<mpptr>&, th, ORBdist) (cslam/src/ORBmatcher.cpp:1478-1604) replayed line by line in Python, the scenes
the tests run it on, and the planted edges.  Written from the source's lines and from OpenCV's rules for the cv::Mat expressions in them, not from this project's
header: numpy.float32 where the source rounds to float, Python floats where it computes in double.

  -Rcw.t()*tcw            one gemm with a transposed operand: a double accumulator over k, alpha = -1, beta = 0, stored to float
  Rcw*x3Dw+tcw            the small-matrix gemm: the three products summed in float, left to right, then (float)((double)t + (double)tcw[i])
  1.0/x3Dc.at<float>(2)   a double quotient stored to a float
  fx*xc*invzc+cx          float, left to right
  x3Dw-Ow, cv::norm       a float difference; the squares summed in double, sqrt in double, stored to a float
  PredictScale            MapPoint.cpp:854-869: ceil(log(ratio)/mfLogScaleFactor) on floats (the C library's logf); a value no int holds converts to INT_MIN on x86,
                          which the clamp turns into level 0
  GetFeaturesInArea       tests/frame_reference.py window_candidates
A frame is a dict(kps, desc, mp, bounds, K); a keyframe a dict(live, pos, dmin, dmax, desc, angle, found)."""
import ctypes as C
import ctypes.util

import numpy as np

import frame_reference as fr

F = np.float32
KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
SKIPPED, OUTSIDE, RANGE, SEARCHED = 0, 1, 2, 3
HISTO_LENGTH = 30
N_LEVELS = 8
W, H = 640, 480
BOUNDS = np.array([0, 0, W, H], np.float32)          # mnMinX mnMinY mnMaxX mnMaxY of an undistorted W x H frame
K_SCENE = np.array([500, 500, 320, 240], np.float32)
K_EDGE = np.array([512, 512, 320, 240], np.float32)  # powers of two: u = 512 x + 320 is exact for the x the edges plant

_libm = C.CDLL(ctypes.util.find_library("m"))
_libm.logf.restype, _libm.logf.argtypes = C.c_float, [C.c_float]


def logf(x):
    return F(_libm.logf(C.c_float(float(x))))


def scale_factors(n=N_LEVELS, s=1.2):
    """mvScaleFactors (ORBextractor.cc): f32, each the previous one times the f32 factor"""
    sf = np.ones(n, np.float32)
    for i in range(1, n):
        sf[i] = F(sf[i - 1] * F(s))
    return sf


SF = scale_factors()
LOG_SF = logf(F(1.2))
IDENTITY = np.eye(4, dtype=np.float32)


def camera_centre(T):
    """:1484"""
    Ow = np.zeros(3, np.float32)
    for r in range(3):
        s = 0.0
        for k in range(3):
            s += float(T[k, r]) * float(T[k, 3])
        Ow[r] = F(s * -1.0 + 0.0)
    return Ow


def predict_scale(dmax, dist, log_sf, n_levels):
    with np.errstate(all="ignore"):
        ratio = F(F(dmax) / F(dist))
        q = F(logf(ratio) / F(log_sf))
    c = np.ceil(q)
    n = int(c) if np.isfinite(c) and -2.0 ** 31 <= c < 2.0 ** 31 else -2 ** 31
    if n < 0:
        n = 0
    elif n >= n_levels:
        n = n_levels - 1
    return n


def gates(T, K, bounds, kf, th, sf=SF, log_sf=LOG_SF, n_levels=N_LEVELS):
    """:1494-1532 for every slot: (status, u, v, level, radius, zc)"""
    T = np.asarray(T, np.float32).reshape(-1)[:12].reshape(3, 4)
    fx, fy, cx, cy = (F(k) for k in K)
    minX, minY, maxX, maxY = (F(b) for b in bounds)
    Ow = camera_centre(T)
    P = len(kf["live"])
    status, u, v = np.zeros(P, np.uint8), np.zeros(P, np.float32), np.zeros(P, np.float32)
    level, radius, zc = np.zeros(P, np.int32), np.full(P, -1, np.float32), np.zeros(P, np.float32)
    found = kf.get("found")
    with np.errstate(all="ignore"):
        for i in range(P):
            if not kf["live"][i] or (found is not None and found[i]):
                continue
            x = kf["pos"][i].astype(np.float32)
            c = np.zeros(3, np.float32)
            for r in range(3):
                t = F(F(F(T[r, 0] * x[0]) + F(T[r, 1] * x[1])) + F(T[r, 2] * x[2]))
                c[r] = F(float(t) + float(T[r, 3]))
            zc[i] = c[2]
            invzc = F(np.float64(1.0) / np.float64(c[2]))
            u[i] = F(F(F(fx * c[0]) * invzc) + cx)
            v[i] = F(F(F(fy * c[1]) * invzc) + cy)
            status[i] = OUTSIDE
            if u[i] < minX or u[i] > maxX:
                continue
            if v[i] < minY or v[i] > maxY:
                continue
            PO = (x - Ow).astype(np.float32)
            s2 = 0.0
            for k in range(3):
                s2 += float(PO[k]) * float(PO[k])
            dist3D = F(np.sqrt(np.float64(s2)))
            status[i] = RANGE
            if dist3D < F(F(0.8) * kf["dmin"][i]) or dist3D > F(F(1.2) * kf["dmax"][i]):
                continue
            status[i] = SEARCHED
            level[i] = predict_scale(kf["dmax"][i], dist3D, log_sf, n_levels)
            radius[i] = F(F(th) * sf[level[i]])
    return status, u, v, level, radius, zc


def three_maxima(hist):
    """:1607-1648"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, h in enumerate(hist):
        s = len(h)
        if s > max1:
            max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, i
        elif s > max2:
            max3, max2, ind3, ind2 = max2, s, ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < F(0.1) * F(max1):
        ind2 = ind3 = -1
    elif max3 < F(0.1) * F(max1):
        ind3 = -1
    return ind1, ind2, ind3


def replay(frame, T, kf, th, orb_dist, check_orientation=True):
    """The whole function.  Returns dict(status, u, v, level, off, idx, dist, mp, nmatches, removed, zc): off / idx / dist the window candidates of every slot (empty
    where the slot does not reach GetFeaturesInArea), mp = CurrentFrame.mvpMapPoints afterwards (a slot or -1), removed = matches the rotation check took back."""
    kps = frame["kps"]
    status, u, v, level, radius, zc = gates(T, frame["K"], frame["bounds"], kf, th)
    off, idx = fr.window_candidates(frame["bounds"], kps["x"], kps["y"], kps["octave"], u, v, radius, level - 1, level + 1)   # radius -1: no window
    dist = np.zeros(idx.size, np.uint16)
    mp = np.array(frame["mp"], np.int32).copy()
    hist = [[] for _ in range(HISTO_LENGTH)]
    factor = F(1.0) / F(HISTO_LENGTH)
    nmatches = 0
    for i in range(len(status)):
        if off[i + 1] > off[i]:
            dist[off[i]:off[i + 1]] = fr.hamming(kf["desc"][i], frame["desc"][idx[off[i]:off[i + 1]]])
        best_dist, best_idx2 = 256, -1
        for s in range(off[i], off[i + 1]):
            i2 = int(idx[s])
            if mp[i2] >= 0:
                continue
            if int(dist[s]) < best_dist:
                best_dist, best_idx2 = int(dist[s]), i2
        if best_dist <= orb_dist:
            mp[best_idx2] = i
            nmatches += 1
            if check_orientation:
                rot = F(F(kf["angle"][i]) - F(kps["angle"][best_idx2]))
                if rot < 0.0:
                    rot = F(rot + F(360.0))
                b = int(fr._round_half_away(F(rot * factor)))
                if b == HISTO_LENGTH:
                    b = 0
                assert 0 <= b < HISTO_LENGTH
                hist[b].append(best_idx2)
    removed = 0
    if check_orientation:
        keep = three_maxima(hist)
        for b in range(HISTO_LENGTH):
            if b not in keep:
                for i2 in hist[b]:
                    mp[i2] = -1
                    nmatches -= 1
                    removed += 1
    return dict(status=status, u=u, v=v, level=level, off=off, idx=idx, dist=dist, mp=mp, nmatches=nmatches, removed=removed, zc=zc)


# ---- builders -------------------------------------------------------------------------------------------------------------------------------------------
def make_frame(feats, K=K_SCENE, mp=None):
    """feats: rows (x, y, octave, angle, desc[32])"""
    n = len(feats)
    kps = np.zeros(n, KP_DTYPE)
    desc = np.zeros((n, 32), np.uint8)
    for i, (x, y, o, a, d) in enumerate(feats):
        kps[i] = (x, y, 31.0, a, 0.0, o)
        desc[i] = d
    return dict(kps=kps, desc=desc, mp=np.full(n, -1, np.int32) if mp is None else np.asarray(mp, np.int32), bounds=BOUNDS, K=np.asarray(K, np.float32))


def make_kf(points, found=None):
    """points: rows (pos[3], dmin, dmax, desc[32], angle, live)"""
    n = len(points)
    kf = dict(live=np.zeros(n, np.uint8), pos=np.zeros((n, 3), np.float32), dmin=np.zeros(n, np.float32), dmax=np.zeros(n, np.float32),
              desc=np.zeros((n, 32), np.uint8), angle=np.zeros(n, np.float32), found=None if found is None else np.asarray(found, np.uint8))
    for i, (p, a, b, d, ang, live) in enumerate(points):
        kf["pos"][i], kf["dmin"][i], kf["dmax"][i], kf["desc"][i], kf["angle"][i], kf["live"][i] = p, a, b, d, ang, live
    return kf


def flip_bits(desc, k, rng=None, first=0):
    """desc with k bits flipped: bits first .. first + k - 1, or k random ones"""
    d = np.array(desc, np.uint8).copy()
    bits = rng.choice(256, k, replace=False) if rng is not None else range(first, first + k)
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose(rx, ry, rz, t):
    T = np.eye(4)
    T[:3, :3] = rotation(rx, ry, rz)
    T[:3, 3] = t
    return T.astype(np.float32)


def random_scene(seed, P=220, n_clutter=120):
    """A keyframe of P slots and a frame around the projections of its points: (frame, T, kf).  The slots cycle through the kinds the search has to tell apart; the
    frame gets, for most searched slots, a feature near the projection at the predicted level whose descriptor is the point's with a few bits flipped and whose angle
    puts the match into one of three rotation bins (a few into stray bins, for the rotation check to take back), and clutter."""
    rng = np.random.default_rng(seed)
    T = pose(*rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.2, 0.2, 3))
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    Ow = -R.T @ t
    points = []
    for i in range(P):
        kind = i % 11
        z = rng.uniform(2.0, 8.0)
        if kind == 7:                                   # behind the camera, inside the image
            z = -z
        x = rng.uniform(-0.55, 0.55) * z
        y = rng.uniform(-0.4, 0.4) * z
        if kind == 8:                                   # beside the image
            x = rng.choice([-1.0, 1.0]) * rng.uniform(0.8, 2.0) * abs(z)
        Xc = np.array([x, y, z])
        Xw = R.T @ (Xc - t)
        d = np.linalg.norm(Xw - Ow)
        dmax = d * 1.2 ** rng.uniform(0.0, 7.5)
        dmin = dmax / 1.2 ** 7
        if kind == 9:                                   # too far / too near for the pyramid
            dmax, dmin = (d / 1.5, d / 6.0) if i % 2 else (d * 9.0, d * 1.5)
        live = 0 if kind == 10 else 1
        points.append((Xw, dmin, dmax, rng.integers(0, 256, 32, dtype=np.uint8), rng.uniform(0, 360), live))
    found = np.zeros(P, np.uint8)
    found[5::22] = 1
    kf = make_kf(points, found)
    status, u, v, level, radius, _ = gates(T, K_SCENE, BOUNDS, kf, 10.0)
    feats = []
    for i in np.nonzero(status == SEARCHED)[0]:
        if i % 5 == 4:
            continue                                    # no feature for this slot
        rot = [33.0, 64.0, 95.0][i % 3] if i % 13 else [155.0, 215.0, 275.0, 340.0][(i // 13) % 4]
        r = min(float(radius[i]), 12.0) * 0.6
        feats.append((u[i] + rng.uniform(-r, r), v[i] + rng.uniform(-r, r), int(np.clip(level[i] + rng.integers(-1, 2), 0, N_LEVELS - 1)),
                      (kf["angle"][i] - rot + rng.uniform(-3, 3)) % 360.0, flip_bits(kf["desc"][i], int(rng.integers(0, 40)), rng)))
        if i % 7 == 0:                                  # a second, worse candidate in the window
            feats.append((u[i] + rng.uniform(-r, r), v[i] + rng.uniform(-r, r), int(level[i]), rng.uniform(0, 360), flip_bits(kf["desc"][i], 60, rng)))
    for _ in range(n_clutter):
        feats.append((rng.uniform(-5, W + 5), rng.uniform(-5, H + 5), int(rng.integers(0, N_LEVELS)), rng.uniform(0, 360), rng.integers(0, 256, 32, dtype=np.uint8)))
    order = rng.permutation(len(feats))
    frame = make_frame([feats[j] for j in order])
    frame["mp"][rng.choice(len(feats), 10, replace=False)] = 1000   # features that hold a map point already
    return frame, T, kf


# ---- planted edges: (name, frame, T, kf, th, orb_dist, check_orientation, expect) — expect(r) asserts on the REPLAY's result r what the edge is about ------------------
D0 = np.arange(32, dtype=np.uint8) * 7 + 3     # a descriptor
FAR = 1e3                                      # a distance no point of the edges exceeds


def _pt(pos, dmin=0.1, dmax=4.0, desc=D0, angle=0.0, live=1):
    return (np.asarray(pos, np.float32), dmin, dmax, desc, angle, live)


def _ft(x, y, octave=0, angle=0.0, desc=D0):
    return (x, y, octave, angle, desc)


def _up(x):
    return np.nextafter(F(x), F(np.inf))


def _down(x):
    return np.nextafter(F(x), F(-np.inf))


def edge_cases():
    cases = []

    def add(name, feats, points, expect, th=10.0, orb_dist=100, ori=False, mp=None, found=None):
        cases.append((name, make_frame(feats, K_EDGE, mp), IDENTITY, make_kf(points, found), th, orb_dist, ori, expect))

    # u at the bounds and one ulp beyond: with the identity pose and z = 1, u = 512 x + 320 exactly
    xs = [F(-0.625), _down(-0.625), F(0.625), F(0.625) + F(2.0 ** -23)]

    def e_bounds(r):
        assert r["u"][0] == 0.0 and r["u"][1] == F(-2.0 ** -15) and r["u"][2] == 640.0 and r["u"][3] == _up(640.0)
        assert list(r["status"]) == [SEARCHED, OUTSIDE, SEARCHED, OUTSIDE] and r["nmatches"] == 2
    add("u_at_the_bounds", [_ft(2.0, 240.0), _ft(632.0, 240.0)], [_pt((x, 0, 1), dmax=1.0) for x in xs], e_bounds)
    ys = [F(-0.46875), _down(-0.46875), F(0.46875), F(0.46875) + F(2.0 ** -24)]

    def e_vbounds(r):
        assert r["v"][0] == 0.0 and r["v"][1] < 0.0 and r["v"][2] == 480.0 and r["v"][3] == _up(480.0)
        assert list(r["status"]) == [SEARCHED, OUTSIDE, SEARCHED, OUTSIDE]
    add("v_at_the_bounds", [_ft(320.0, 2.0)], [_pt((0, y, 1), dmax=1.0) for y in ys], e_vbounds)

    # dist3D at each limit and one ulp beyond: the point on the axis at the limit itself
    lo, hi = F(F(0.8) * F(5.0)), F(F(1.2) * F(3.0))

    def e_range(r):
        assert list(r["status"]) == [SEARCHED, RANGE, SEARCHED, RANGE]
    add("dist_at_the_limits", [_ft(320.0, 240.0)], [_pt((0, 0, lo), 5.0, FAR), _pt((0, 0, _down(lo)), 5.0, FAR), _pt((0, 0, hi), 0.1, 3.0), _pt((0, 0, _up(hi)), 0.1, 3.0)],
        e_range)

    # z == 0: x / 0 = inf is outside; 0 * inf = NaN passes the image test, and with mfMinDistance = 0 the distance test too: level 0, an empty window
    def e_z0(r):
        assert np.isinf(r["u"][0]) and r["status"][0] == OUTSIDE and np.isnan(r["u"][1]) and np.isnan(r["v"][1]) and r["status"][1] == SEARCHED
        assert r["level"][1] == 0 and r["off"][-1] == 0 and r["status"][2] == RANGE
    add("z_zero", [_ft(320.0, 240.0)], [_pt((1, 1, 0)), _pt((0, 0, 0), 0.0, 4.0), _pt((0, 0, 0), 1.0, 4.0)], e_z0)

    # level 0 (the window's lower level is -1: only the upper bound is tested) and level nlevels - 1
    def e_levels(r):
        assert list(r["level"]) == [0, N_LEVELS - 1]
        assert r["u"][0] == 318.0 and r["u"][1] == 500.0
        assert sorted(r["idx"][r["off"][0]:r["off"][1]]) == [0, 1] and sorted(r["idx"][r["off"][1]:r["off"][2]]) == [4, 5]
    add("first_and_last_level", [_ft(318.0, 240.0, 0), _ft(318.0, 241.0, 1), _ft(318.0, 242.0, 2), _ft(500.0, 240.0, 5), _ft(500.0, 241.0, 6), _ft(500.0, 242.0, 7)],
        [_pt((-0.015625, 0, 4), dmax=3.9), _pt((1.40625, 0, 4), dmax=4.0 * 1.2 ** 10)], e_levels, th=3.0)

    # a window across the grid's rim: the cells left of and above the image do not exist
    def e_rim(r):
        assert r["status"][0] == SEARCHED and r["u"][0] < 2 and r["v"][0] < 2 and sorted(r["idx"]) == [0, 1, 2] and r["nmatches"] == 1
    add("window_across_the_rim", [_ft(0.0, 0.0, 0, 0.0, flip_bits(D0, 9)), _ft(6.0, 1.0, 0, 0.0, flip_bits(D0, 5)), _ft(1.0, 7.0, 1, 0.0, flip_bits(D0, 7)), _ft(14.0, 3.0)],
        [_pt(((1.0 - 320.0) / 512.0, (1.0 - 240.0) / 512.0, 1), dmax=1.3)], e_rim)

    # a distance tie: the first in GetFeaturesInArea's order wins, which is the cell order, not the feature index
    def e_tie(r):
        assert list(r["idx"]) == [1, 0] and r["dist"][0] == r["dist"][1] == 6 and r["mp"][1] == 0 and r["mp"][0] == -1
    add("distance_tie", [_ft(330.0, 240.0, 0, 0.0, flip_bits(D0, 6, first=40)), _ft(310.0, 240.0, 0, 0.0, flip_bits(D0, 6))], [_pt((0, 0, 4), dmax=4.0)], e_tie, th=15.0)

    # two points wanting the same feature: the first slot claims it, the second takes the next best
    def e_claim(r):
        assert r["mp"][0] == 0 and r["mp"][1] == 1 and r["nmatches"] == 2 and r["dist"][r["off"][1]] < r["dist"][r["off"][1] + 1]
    add("two_points_one_feature", [_ft(320.0, 240.0, 0, 0.0, flip_bits(D0, 2)), _ft(322.0, 240.0, 0, 0.0, flip_bits(D0, 30))], [_pt((0, 0, 4)), _pt((0, 0, 4))], e_claim)

    # every candidate holds a map point already, whatever it is
    def e_claimed(r):
        assert r["off"][-1] == 2 and r["nmatches"] == 0 and list(r["mp"]) == [5, 0]
    add("every_candidate_claimed", [_ft(320.0, 240.0), _ft(322.0, 240.0)], [_pt((0, 0, 4))], e_claimed, mp=[5, 0])

    # bestDist <= ORBdist is inclusive
    for od, n in ((10, 1), (9, 0)):
        def e_od(r, n=n):
            assert r["dist"][0] == 10 and r["nmatches"] == n
        add("dist_%s_orbdist_%d" % ("equals" if n else "above", od), [_ft(320.0, 240.0, 0, 0.0, flip_bits(D0, 10))], [_pt((0, 0, 4))], e_od, orb_dist=od)

    # the rotation check: rot < 0 wraps by 360, bin 30 becomes bin 0, the bins beyond the three fullest lose their matches
    rots = [(10.0, 350.0)] * 3 + [(100.0, 10.0)] * 3 + [(150.0, 0.0)] * 3 + [(900.0, 0.0), (3.0, 0.0), (200.0, 350.0)]   # bins 1 (wrapped) | 3 | 5 | 0 (from 30), 0 | 7

    def e_rot(r):
        assert r["removed"] == 3 and r["nmatches"] == 9 and list(r["mp"][9:]) == [-1, -1, -1] and list(r["mp"][:9]) == list(range(9))
    add("rotation_wrap_and_bin_30", [_ft(40.0 + 50 * j, 240.0, 2, fa, flip_bits(D0, j, first=8 * j)) for j, (_, fa) in enumerate(rots)],
        [_pt(((40.0 + 50 * j - 320.0) / 512.0 * 4, 0, 4), dmax=6.0, desc=flip_bits(D0, j, first=8 * j), angle=ka) for j, (ka, _) in enumerate(rots)], e_rot, th=3.0, ori=True)

    # a slot without a live point and a slot in sAlreadyFound are not projected at all
    def e_skip(r):
        assert list(r["status"]) == [SKIPPED, SKIPPED, SEARCHED] and r["off"][2] == 0 and r["mp"][0] == 2 and r["u"][0] == 0 and r["v"][1] == 0
    add("skipped_slots", [_ft(320.0, 240.0)], [_pt((0, 0, 4), live=0), _pt((0, 0, 4)), _pt((0, 0, 4))], e_skip, found=[0, 1, 0])
    return cases


def same_float_bits(a, b):
    """equal bit patterns; a NaN equals a NaN (0 * inf has no payload the source, the host and the device agree on)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


# ---- scenes of the refine chain ---------------------------------------------------------------------------------------------------------------------------
REFINE_PATHS = ("few", "first", "widen1", "widen2")
INV_LEVEL_SIGMA2 = (F(1.0) / (SF * SF)).astype(np.float32)


def refine_scene(path, seed=7, n_slots=150, n_feat=400):
    """A candidate keyframe of n_slots points on a jittered 15 x 10 lattice of projections (no two windows meet), a frame of n_feat features and a PnP pose near
    the true one: dict(frame, kf, T0, matches_f, inliers).  Every feature of a slot lies at the slot's exact projection under the true pose, at octave 1 (the slots
    predict level 1), with the slot's descriptor and an angle that puts the match into a chosen rotation bin; a decoy lies 8 px beside it, inside the first search's
    window and an outlier of the optimisation.  What a path gets:
      few      8 seeds (matches of SearchByBoW that the PnP pose keeps), so the first optimisation ends below 10
      first    60 seeds
      widen1   32 seeds, 40 more slots with a feature for the first search
      widen2   32 seeds; 15 slots with a feature and 12 with a decoy in three rotation bins of 9, and 7 slots with a feature in a fourth bin: the first search's
               rotation check takes those 7 back, the second optimisation ends between 30 and 50, and the second search, alone with them, keeps them"""
    assert path in REFINE_PATHS
    rng = np.random.default_rng(seed)
    T_gt = pose(0.02, -0.03, 0.01, [0.1, -0.05, 0.2])
    T0 = pose(0.022, -0.028, 0.012, [0.11, -0.045, 0.21])
    R, t = T_gt[:3, :3].astype(np.float64), T_gt[:3, 3].astype(np.float64)
    Ow = -R.T @ t
    fx, fy, cx, cy = (float(k) for k in K_SCENE)
    role = np.full(n_slots, "none", object)
    order = rng.permutation(n_slots)
    plan = {"few": [("seed", 8), ("good1", 30)], "first": [("seed", 60), ("good1", 20)], "widen1": [("seed", 32), ("good1", 14), ("good2", 13), ("good3", 13)],
            "widen2": [("seed", 32), ("good1", 5), ("good2", 5), ("good3", 5), ("decoy1", 4), ("decoy2", 4), ("decoy3", 4), ("good5", 7)]}[path]
    at = 0
    for name, n in plan:
        role[order[at:at + n]] = name
        at += n
    points, feats, owner = [], [], []
    for s in range(n_slots):
        gx, gy = s % 15, s // 15
        uu, vv = 40.0 + 40.0 * gx + rng.uniform(-5, 5), 40.0 + 44.0 * gy + rng.uniform(-5, 5)
        z = rng.uniform(3.0, 6.0)
        Xw = (R.T @ (np.array([(uu - cx) / fx * z, (vv - cy) / fy * z, z]) - t)).astype(np.float32)
        d = np.linalg.norm(Xw.astype(np.float64) - Ow)
        desc, ang = rng.integers(0, 256, 32, dtype=np.uint8), rng.uniform(0, 360)
        points.append((Xw, d * 1.1 / 1.2 ** 7, d * 1.1, desc, ang, 1))
        if role[s] == "none":
            continue
        Xc = R @ Xw.astype(np.float64) + t
        pu, pv = fx * Xc[0] / Xc[2] + cx, fy * Xc[1] / Xc[2] + cy
        if role[s].startswith("decoy"):
            pu += 8.0
        b = 1 if role[s] == "seed" else int(role[s][-1])
        feats.append((pu, pv, 1, (ang - (30.0 * b + 4.0)) % 360.0, flip_bits(desc, int(rng.integers(0, 20)), rng)))
        owner.append(s if role[s] == "seed" else -1)
    while len(feats) < n_feat:
        feats.append((rng.uniform(0, W), rng.uniform(0, H), int(rng.integers(0, N_LEVELS)), rng.uniform(0, 360), rng.integers(0, 256, 32, dtype=np.uint8)))
        owner.append(-1)
    perm = rng.permutation(n_feat)
    frame = make_frame([feats[j] for j in perm])
    matches_f = np.array([owner[j] for j in perm], np.int32)
    inliers = (matches_f >= 0).astype(np.uint8)
    loose = np.nonzero(matches_f < 0)[0][:5]            # matches of SearchByBoW that the PnP pose rejected: they seed nothing
    matches_f[loose] = order[-5:]
    return dict(frame=frame, kf=make_kf(points), T0=T0, matches_f=matches_f, inliers=inliers)


# ---- what the CPU and the GPU tests share: the scenes' arrays as the wrappers of ccm_slam_amd.reloc take them, and the comparison of an evaluation ----------------
def _reloc():
    from ccm_slam_amd import reloc
    return reloc


def pose_of(T):
    return _reloc().guided_pose(T, LOG_SF, SF)


def kf_of(kf):
    return _reloc().KeyFramePoints(kf["live"], kf["pos"], kf["dmin"], kf["dmax"], kf["desc"], kf["angle"])


def skip_of(kf):
    s = (kf["live"] == 0)
    return (s | (kf["found"] != 0) if kf["found"] is not None else s).astype(np.uint8)


def assert_evaluation(got, r, what):
    for k in ("status", "level", "off", "idx", "dist"):
        assert np.array_equal(got[k], r[k]), (what, k)
    assert same_float_bits(got["u"], r["u"]) and same_float_bits(got["v"], r["v"]), what
    assert got["n_cand"] == r["idx"].size, what


def host_eval(frame, T, kf, th):
    return _reloc().guided_search_host(frame["kps"], frame["desc"], frame["bounds"], frame["K"], pose_of(T), kf["pos"], kf["dmin"], kf["dmax"], kf["desc"], skip_of(kf), th)


def host_mirror(frame, T, kf, th, orb_dist, ori):
    return _reloc().search_by_projection_kf_host(frame["kps"], frame["desc"], frame["bounds"], frame["K"], pose_of(T), kf_of(kf), kf["found"], th, orb_dist, ori, frame["mp"])
