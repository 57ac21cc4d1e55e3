"""The inputs of tests/test_frame_edges_gpu.py, built once and shared with tests/test_frame_reference_cpu.py, which checks on the CPU that the reference
agrees with the oracle on them and that every case really stands where it claims to (a tie is a tie, a 17-cell window has 17 cells, a planted pair straddles
its threshold).  Keypoints are synthetic: seeded f32 positions on an undistorted 752 x 480 frame, so that positions reach the grid exactly as written."""
import ctypes as C
import ctypes.util

import numpy as np

import frame_reference as fr

F = np.float32
EUROC_K = np.array([458.654, 457.296, 367.215, 248.375], np.float32)
W, H = 752, 480
BOUNDS = (F(0), F(0), F(W), F(H))                      # mnMinX mnMinY mnMaxX mnMaxY of an undistorted frame
KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
INF, NAN = F(np.inf), F(np.nan)


def make_kps(x, y, seed):
    """(keypoints, descriptors): the given positions, octaves 0..7 and descriptors drawn from the seed"""
    rng = np.random.default_rng(seed)
    x = np.asarray(x, np.float32)
    kps = np.zeros(x.size, KP_DTYPE)
    kps["x"], kps["y"] = x, np.asarray(y, np.float32)
    kps["size"], kps["angle"], kps["response"] = 31.0, 0.0, 1.0
    kps["octave"] = rng.integers(0, 8, x.size)
    return kps, rng.integers(0, 256, (x.size, 32), dtype=np.uint8)


def uniform_kps(n, seed, margin=12.0):
    """n keypoints over the image and a margin around it (the ones in the margin's outer part fall out of the grid)"""
    rng = np.random.default_rng(seed)
    return make_kps(rng.uniform(-margin, W + margin, n), rng.uniform(-margin, H + margin, n), seed + 1)


# ---- grid -----------------------------------------------------------------------------------------------------------------------------------------------
GRID_SIZES = (1, 1023, 1024, 1025, 2048, 2049, 3100, 5)   # one handle, in this order: second trip of the stride loops, growth past 2048, reuse at a smaller N


def grid_size_kps(n):
    """the keypoints of one grid size; the sizes 1 and 5 lie wholly inside the image (all of them are placed)"""
    return uniform_kps(n, 1000 + n, margin=-20.0 if n <= 5 else 12.0)


def crowded_case():
    """1500 keypoints, 500 in each of the cells (0, 0), (37, 23), (74, 47), their indices interleaved at random"""
    rng = np.random.default_rng(11)
    wInv, hInv = fr.grid_inverses(BOUNDS)
    cx = np.repeat([0, 37, 74], 500); cy = np.repeat([0, 23, 47], 500)
    x = (cx + rng.uniform(-0.4, 0.4, 1500)) / float(wInv)
    y = (cy + rng.uniform(-0.4, 0.4, 1500)) / float(hInv)
    p = rng.permutation(1500)
    return make_kps(x[p], y[p], 12), (cx[p] * fr.GRID_ROWS + cy[p])


def rim_case(wild=False):
    """every pairing of rim / outside values in x with the same in y.  wild: with coordinates whose grid product no int holds (the source's conversion is
    undefined there and the oracle restates it, so these are judged by the reference alone: in no cell)."""
    xs = [0.0, -0.0, np.nextafter(F(0), F(-1)), 5.0, W, np.nextafter(F(W), F(0)), np.nextafter(F(W), F(2 * W)), 747.0, -1.0, -5.1, -300.0, 760.0, 1e6, -1e6]
    ys = [0.0, -0.0, 4.9, 5.0, H, np.nextafter(F(H), F(0)), np.nextafter(F(H), F(2 * H)), 475.0, -1.0, -5.1, 500.0, 1e6]
    if wild:
        xs += [3e38, -3e38, np.inf, -np.inf, np.nan]; ys += [-3e38, np.inf, np.nan]
    X, Y = np.meshgrid(np.array(xs, np.float32), np.array(ys, np.float32), indexing="ij")
    return make_kps(X.ravel(), Y.ravel(), 13)


def find_ties(inv, n_cells):
    """[(k, c)]: for every cell k < n_cells an f32 coordinate c with f32(c * inv) == k + 0.5 exactly, where one exists among the f32 neighbours of (k + 0.5) / inv"""
    out = []
    for k in range(n_cells):
        c = F((k + 0.5) / float(inv))
        cands = [c]
        lo = hi = c
        for _ in range(16):
            lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
            cands += [lo, hi]
        hit = [a for a in cands if F(a * inv) == F(k + 0.5)]
        if hit:
            out.append((k, hit[0]))
    return out


def tie_case():
    """keypoints whose grid product is k + 0.5 exactly, in x (at y = 123.25) and in y (at x = 301.75): round() takes each to cell k + 1.
    Returns (kps, desc), the expected cell of every keypoint by the half-away rule stated in integers, and the tie lists."""
    wInv, hInv = fr.grid_inverses(BOUNDS)
    tx, ty = find_ties(wInv, fr.GRID_COLS), find_ties(hInv, fr.GRID_ROWS)
    x = [c for _, c in tx] + [301.75] * len(ty)
    y = [123.25] * len(tx) + [c for _, c in ty]
    iy0 = int(np.floor(123.25 * float(hInv) + 0.5)); ix0 = int(np.floor(301.75 * float(wInv) + 0.5))   # far from a tie themselves
    exp = [(k + 1) * fr.GRID_ROWS + iy0 if k + 1 < fr.GRID_COLS else -1 for k, _ in tx] + [ix0 * fr.GRID_ROWS + k + 1 if k + 1 < fr.GRID_ROWS else -1 for k, _ in ty]
    return make_kps(x, y, 14), np.array(exp, np.int64), tx, ty


# ---- window search --------------------------------------------------------------------------------------------------------------------------------------
LEVEL_PAIRS = ((-1, -1), (0, -1), (0, 0), (3, -1), (2, 5), (5, 2), (7, 7))
QUERY_COUNTS = (1, 7, 8, 9, 1023, 1024, 1025, 2049)


def query_count_case():
    """2000 keypoints and 2049 queries with mixed radii and level windows; a test with Q queries takes the first Q (a prefix's lists are the prefix of the lists)"""
    kps, desc = uniform_kps(2000, 21)
    rng = np.random.default_rng(22)
    Q = 2049
    u = rng.uniform(-40, W + 40, Q).astype(np.float32); v = rng.uniform(-40, H + 40, Q).astype(np.float32)
    r = rng.choice(np.array([0.0, 2.5, 7.0, 15.0, 40.0, 130.0], np.float32), Q)
    lv = np.array(LEVEL_PAIRS, np.int32)[rng.integers(0, len(LEVEL_PAIRS), Q)]
    return kps, desc, dict(u=u, v=v, r=r, minl=lv[:, 0].copy(), maxl=lv[:, 1].copy(), qdesc=rng.integers(0, 256, (Q, 32), dtype=np.uint8))


def _find_window(n_cells, v, r, probe_dx, probe_y):
    """a u whose window (u, v, r) covers exactly n_cells cells, the keypoint (u + probe_dx, probe_y) lying in the window's LAST column"""
    for u in np.arange(300.0, 340.0, 0.125, dtype=np.float32):
        rg = fr.cell_range(BOUNDS, u, v, r)
        if rg and (rg[1] - rg[0] + 1) * (rg[3] - rg[2] + 1) == n_cells and fr.cell_of(BOUNDS, F(u + F(probe_dx)), probe_y)[0] // fr.GRID_ROWS == rg[1]:
            return F(u)
    raise AssertionError(f"no window of {n_cells} cells")


A_IDX, B_IDX, C_IDX, D_IDX = 2000, 2001, 2002, 2003     # the planted keypoints of window_shape_case


def window_shape_case():
    """2000 uniform keypoints plus A = (300, 200), B = (412.5, 100.25), C in the last column of the 16-cell window (4 x 4) and D in the last (17th) cell of the
    17-cell window (17 x 1); one query per row, named"""
    kps, desc = uniform_kps(2000, 31)
    u16 = _find_window(16, 105.0, 10.0, 9.5, 114.5)                   # 4 x 4
    u17 = _find_window(17, 550.0, 80.0, 79.5, 472.0)                  # 17 columns of the bottom row: the window's centre lies below the image
    k2, d2 = make_kps([300.0, 412.5, u16 + F(9.5), u17 + F(79.5)], [200.0, 100.25, 114.5, 472.0], 32)
    kps, desc = np.concatenate([kps, k2]), np.concatenate([desc, d2])
    rows = [("r0_on_keypoint", 300.0, 200.0, 0.0),
            ("dx_equals_r", 400.0, 100.25, 12.5), ("dx_below_next_r", 400.0, 100.25, np.nextafter(F(12.5), INF)),
            ("cells_16", u16, 105.0, 10.0), ("cells_17", u17, 550.0, 80.0), ("whole_grid", 376.0, 240.0, 2000.0),
            ("corner_00", 0.0, 0.0, 30.0), ("corner_w0", W, 0.0, 30.0), ("corner_0h", 0.0, H, 30.0), ("corner_wh", W, H, 30.0),
            ("left_of", -100.0, 240.0, 50.0), ("right_of", 900.0, 240.0, 50.0), ("above", 376.0, -100.0, 50.0), ("below", 376.0, 600.0, 50.0),
            ("straddle_left", -10.0, 240.0, 30.0), ("straddle_right", 760.0, 240.0, 30.0), ("straddle_top", 376.0, -10.0, 30.0), ("straddle_bottom", 376.0, 490.0, 30.0)]
    names = [n for n, *_ in rows]
    u, v, r = (np.array([row[i] for row in rows], np.float32) for i in (1, 2, 3))
    Q = len(rows)
    rng = np.random.default_rng(33)
    q = dict(u=u, v=v, r=r, minl=np.full(Q, -1, np.int32), maxl=np.full(Q, -1, np.int32), qdesc=rng.integers(0, 256, (Q, 32), dtype=np.uint8))
    return kps, desc, q, {n: i for i, n in enumerate(names)}


def level_case():
    """one window around the image centre under every level pair of LEVEL_PAIRS"""
    kps, desc = uniform_kps(2000, 41)
    Q = len(LEVEL_PAIRS)
    lv = np.array(LEVEL_PAIRS, np.int32)
    rng = np.random.default_rng(42)
    return kps, desc, dict(u=np.full(Q, 371.5, np.float32), v=np.full(Q, 236.25, np.float32), r=np.full(Q, 90.0, np.float32), minl=lv[:, 0].copy(), maxl=lv[:, 1].copy(),
                           qdesc=rng.integers(0, 256, (Q, 32), dtype=np.uint8))


BAD_UV = (NAN, INF, -INF)
BAD_R = (NAN, F(-1), F(-100), INF, F(1e12), F(3e38))


def total_range_case():
    """32 queries = four blocks of 8: every odd slot holds a query outside the source's defined domain, every even slot an ordinary one.  The r < 0 rows include
    (376, 235, -240), whose unchecked range is y0 = 47, y1 = 0 with x1 < x0.  Returns the queries and the mask of the ordinary ones."""
    kps, desc = uniform_kps(2000, 51)
    bad = [(b, 200.0, 25.0) for b in BAD_UV] + [(300.0, b, 25.0) for b in BAD_UV] + [(376.0, 240.0, b) for b in BAD_R] + \
          [(376.0, 235.0, -240.0), (INF, 240.0, INF), (-INF, INF, INF), (NAN, NAN, NAN)]
    rng = np.random.default_rng(52)
    rows, ordinary = [], []
    for i in range(max(len(bad), 12)):
        rows.append((rng.uniform(0, W), rng.uniform(0, H), rng.choice([25.0, 60.0, 90.0]))); ordinary.append(True)
        rows.append(bad[i % len(bad)]); ordinary.append(False)
    u, v, r = (np.array([row[i] for row in rows], np.float32) for i in (0, 1, 2))
    Q = len(rows)
    q = dict(u=u, v=v, r=r, minl=np.full(Q, -1, np.int32), maxl=np.full(Q, -1, np.int32), qdesc=rng.integers(0, 256, (Q, 32), dtype=np.uint8))
    return kps, desc, q, np.array(ordinary)


def take(q, sel):
    return {k: np.ascontiguousarray(a[sel]) for k, a in q.items()}


# ---- frustum --------------------------------------------------------------------------------------------------------------------------------------------
N_LEVELS = 8
LOG_SF = F(np.log(F(1.2)))
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype, _libm.logf.argtypes = C.c_float, [C.c_float]


def logf(x):
    """the C library's logf, which is what MapPoint::PredictScale calls"""
    return F(_libm.logf(C.c_float(float(x))))


def frame24(R, t, K4, b4):
    """Rcw 9 | tcw 3 | Ow 3 | fx fy cx cy | minX maxX minY maxY | log(scale factor), with Ow = -R^T t"""
    R, t = np.asarray(R, np.float32), np.asarray(t, np.float32)
    Ow = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(np.float32)
    return np.concatenate([R.ravel(), t, Ow, np.asarray(K4, np.float32), np.asarray(b4, np.float32), [LOG_SF]]).astype(np.float32)


TABLE_FRAME = frame24(np.eye(3), np.zeros(3), [512, 512, 256, 256], [0, 512, 0, 512])


def level_ratio_rows():
    """[(k, dmax)] at dist = 4: f32 dmax near 4 * 1.2^k whose level quotient f32(logf(dmax / 4) / logSF) is the integer k exactly, so that ceil() gives k and the
    first float above whose quotient differs gives k + 1.  k = 0 is dmax = 4 (ratio 1, logf = 0)."""
    out = [(0, F(4.0))]
    for k in range(1, 12):
        c = F(4.0 * 1.2 ** k)
        cands = [c]; lo = hi = c
        for _ in range(8):
            lo, hi = np.nextafter(lo, F(0)), np.nextafter(hi, INF)
            cands += [lo, hi]
        hit = [d for d in cands if F(logf(F(d / F(4.0))) / LOG_SF) == F(k)]
        if hit:
            out.append((k, hit[0]))
    return out


def frustum_table():
    """rows (name, P, Pn, dmin, dmax, in_view expected, level expected or None) on TABLE_FRAME; every row sits ON one comparison's equality.  The precondition each
    row relies on is checked in f32 by check_frustum_table()."""
    z = (0.0, 0.0, 1.0)
    rows = [("u_eq_minX", (-2.0, 0.0, 4.0), z, 0.1, 8.0, 1, None), ("u_eq_maxX", (2.0, 0.0, 4.0), z, 0.1, 8.0, 1, None),
            ("v_eq_minY", (0.0, -2.0, 4.0), z, 0.1, 8.0, 1, None), ("v_eq_maxY", (0.0, 2.0, 4.0), z, 0.1, 8.0, 1, None),
            # Pc.z == +-0 passes `Pc.z < 0`; with the point ON the camera centre dist is 0 and the projection is 0 * inf: every later comparison sees a NaN or 0 and
            # lets it through (dmin = 0), and PredictScale's log(1 / 0) = inf is converted as the source's x86 build converts it (INT_MIN, clamped to level 0)
            ("z_plus_zero", (0.0, 0.0, 0.0), z, 0.0, 1.0, 1, 0), ("z_minus_zero", (0.0, 0.0, -0.0), z, 0.0, 1.0, 1, 0),
            ("z_least_negative", (0.0, 0.0, -float(np.nextafter(F(0), F(1)))), z, 0.0, 1.0, 0, None),
            ("dist_eq_max", (0.0, 0.0, 3.0), z, 0.1, 2.5, 1, None), ("dist_eq_min", (0.0, 0.0, 4.0), z, 5.0, 8.0, 1, None),
            ("cos_eq_limit", (0.0, 0.0, 4.0), (0.0, 0.0, 0.5), 0.1, 8.0, 1, None),
            ("ratio_below_1", (0.0, 0.0, 4.0), z, 0.1, 3.5, 1, 0), ("ratio_clamps", (0.0, 0.0, 4.0), z, 0.1, 400.0, 1, N_LEVELS - 1)]
    for k, dmax in level_ratio_rows():
        rows.append((f"ratio_pow_{k}", (0.0, 0.0, 4.0), z, 0.1, float(dmax), 1, min(k, N_LEVELS - 1)))
        up = np.nextafter(dmax, INF)
        while F(logf(F(up / F(4.0))) / LOG_SF) == F(k):             # the quotient is rounded too: the first float whose quotient exceeds k
            up = np.nextafter(up, INF)
        rows.append((f"ratio_pow_{k}_next", (0.0, 0.0, 4.0), z, 0.1, float(up), 1, min(k + 1, N_LEVELS - 1)))
    return rows


def table_arrays(rows):
    P = np.array([r[1] for r in rows], np.float32); Pn = np.array([r[2] for r in rows], np.float32)
    return P, Pn, np.array([r[3] for r in rows], np.float32), np.array([r[4] for r in rows], np.float32)


def check_frustum_table(rows):
    """the equalities the table claims, in NumPy f32"""
    by = {r[0]: r for r in rows}
    fx = cx = F(512); c0 = F(256)
    for name, axis, edge in (("u_eq_minX", 0, 0.0), ("u_eq_maxX", 0, 512.0), ("v_eq_minY", 1, 0.0), ("v_eq_maxY", 1, 512.0)):
        P = np.array(by[name][1], np.float32)
        assert F(F(fx * P[axis]) * F(F(1) / P[2])) + c0 == F(edge), name
    assert np.signbit(F(by["z_minus_zero"][1][2])) and F(by["z_minus_zero"][1][2]) == 0 and not np.signbit(F(by["z_plus_zero"][1][2]))
    assert F(by["z_least_negative"][1][2]) < 0 and np.nextafter(F(by["z_least_negative"][1][2]), F(1)) == 0
    assert F(F(1.2) * F(2.5)) == F(3.0) and F(np.sqrt(np.float64(3.0) ** 2)) == F(3.0)                     # dist == 1.2f * dmax
    assert F(F(0.8) * F(5.0)) == F(4.0)                                                                  # dist == 0.8f * dmin
    assert F(np.float64(F(4.0)) * np.float64(F(0.5)) / np.float64(F(4.0))) == F(0.5)                      # viewCos == 0.5
    pows = [r for r in rows if r[0].startswith("ratio_pow_") and not r[0].endswith("_next")]
    for r in pows:
        k = int(r[0].split("_")[2])
        assert F(logf(F(F(r[4]) / F(4.0))) / LOG_SF) == F(k), r[0]
    assert len(pows) >= 4, [r[0] for r in pows]                                                          # ratio 1 and at least three powers
    assert F(3.5) / F(4.0) < 1 and np.ceil(F(logf(F(100.0)) / LOG_SF)) > N_LEVELS


def frustum_random_case(n, seed):
    """n points around a camera on a tilted pose, in the manner of tests/test_frame_gpu.py: every branch is taken"""
    rng = np.random.default_rng(seed)
    a, b = 0.3, -0.2
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]); Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    fr24 = frame24(Rx @ Ry, [0.4, -0.3, 0.2], EUROC_K, [-135.79564, 895.5073, -92.875015, 565.5531])
    Ow = fr24[12:15]
    P = (Ow + rng.normal(size=(n, 3)) * 6).astype(np.float32)
    view = P - Ow
    nrm = view / np.linalg.norm(view, axis=1, keepdims=True) + rng.normal(size=(n, 3)) * rng.choice([0.05, 0.8], (n, 1))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    dmax = (np.linalg.norm(view, axis=1) * rng.uniform(0.6, 4.0, n)).astype(np.float32)
    return fr24, P, nrm, (dmax / F(1.2 ** 7)).astype(np.float32), dmax


# adjacent floats: the frame is R = I, t != 0 with the EuRoC camera, so that each bisected input is ONE f32 of the call and moves one comparison's left side
PLANT_T = np.array([0.3, -0.2, 0.1], np.float32)
PLANT_BOUNDS = np.array([-135.79564, 895.5073, -92.875015, 565.5531], np.float32)       # minX maxX minY maxY
PLANT_FRAME = frame24(np.eye(3), PLANT_T, EUROC_K, PLANT_BOUNDS)
PLANT_TESTS = ("z_behind", "u_below_minX", "u_above_maxX", "v_below_minY", "v_above_maxY", "dist_below_min", "dist_above_max", "cos_below_limit")
N_PLANT = 64


def _ordered(a):
    """f32 -> int64 keys that ascend with the float (-0.0 and +0.0 are neighbours)"""
    i = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff) - 1, i)


def _unordered(k):
    k = np.asarray(k, np.int64)
    return np.where(k < 0, (-(k + 1)) | 0x80000000, k).astype(np.uint32).view(np.float32)


def plant_adjacent(is_in_frustum, test):
    """For one rejection test: 64 base points in view with margin, one f32 input bisected (vectorised over the points) between a value in view and a value
    rejected, down to two ADJACENT floats on which `is_in_frustum` (the oracle) differs.  Returns (P, Pn, dmin, dmax) of 2 x 64 points (the in-view side first)
    and the mask of the points whose pair stands at this test's own threshold (planted); the others met another rejection first and are dropped by the caller."""
    rng = np.random.default_rng(100 + PLANT_TESTS.index(test))
    n = N_PLANT
    Ow = PLANT_FRAME[12:15]
    # base: camera coordinates well inside the image, depth 2..6; the world point is Pc - t (R = I)
    zc = rng.uniform(2.0, 6.0, n)
    xc = rng.uniform(-0.35, 0.35, n) * zc; yc = rng.uniform(-0.25, 0.25, n) * zc
    if test == "z_behind":
        xc[:] = 0.0; yc[:] = 0.0                     # on the optical axis: Pc.x = Pc.y = 0 exactly, so that u, v stay at (cx, cy) however small the depth gets
    P = (np.stack([xc, yc, zc], 1) - PLANT_T.astype(np.float64)).astype(np.float32)
    if test == "z_behind":
        P[:, 0], P[:, 1] = -PLANT_T[0], -PLANT_T[1]
    d = np.linalg.norm(P.astype(np.float64) - Ow, axis=1)
    Pn = ((P - Ow) / d[:, None]).astype(np.float32)                                       # cos = 1
    edge = {"u_below_minX": (0, PLANT_BOUNDS[0]), "u_above_maxX": (0, PLANT_BOUNDS[1]), "v_below_minY": (1, PLANT_BOUNDS[2]), "v_above_maxY": (1, PLANT_BOUNDS[3])}.get(test)
    if edge:
        # the normal halves the angle between the base direction and the direction at the image's edge (up to 50 degrees apart), so that the angle test keeps its margin
        ax, e = edge
        at_edge = np.stack([xc, yc, zc], 1)
        at_edge[:, ax] = (float(e) - float(EUROC_K[2 + ax])) / float(EUROC_K[ax]) * zc
        mid = (P - Ow) / d[:, None] + at_edge / np.linalg.norm(at_edge, axis=1, keepdims=True)
        Pn = (mid / np.linalg.norm(mid, axis=1, keepdims=True)).astype(np.float32)
    dmax = (d * rng.uniform(1.5, 3.0, n)).astype(np.float32)
    dmin = (d * rng.uniform(0.2, 0.5, n)).astype(np.float32)
    if test == "z_behind":
        dmin[:] = 0.0                                                                       # the depth may shrink to nothing without the distance test firing
        Pn[:] = (0.0, 0.0, 1.0)
    arr = {"P": P, "Pn": Pn, "dmin": dmin, "dmax": dmax}
    # (array, column, value rejected by this test)
    which = {"z_behind": ("P", 2, -PLANT_T[2] - 1.0), "u_below_minX": ("P", 0, -50.0), "u_above_maxX": ("P", 0, 50.0), "v_below_minY": ("P", 1, -50.0),
             "v_above_maxY": ("P", 1, 50.0), "dist_below_min": ("dmin", None, 100.0), "dist_above_max": ("dmax", None, 1e-3), "cos_below_limit": ("Pn", 0, None)}[test]
    name, col, bad = which
    if test == "cos_below_limit":
        # tilt: the normal's lateral component against the side the point lies on; cos = (PO.x * c + PO.y * ny + PO.z * nz) / dist falls as c goes that way
        P[:, 0] = np.where(np.abs(P[:, 0] + PLANT_T[0]) < 0.2, F(0.5) - PLANT_T[0], P[:, 0])
        bad = -np.sign(P[:, 0] - Ow[0]) * 50.0
    get = (lambda: arr[name]) if col is None else (lambda: arr[name][:, col])
    good_k = _ordered(get().copy())
    bad_k = _ordered(np.broadcast_to(np.asarray(bad, np.float32), (n,)).copy())

    def flag(keys):
        a = {k: v.copy() for k, v in arr.items()}
        if col is None:
            a[name] = _unordered(keys)
        else:
            a[name][:, col] = _unordered(keys)
        return a, is_in_frustum(PLANT_FRAME, N_LEVELS, a["P"], a["Pn"], a["dmin"], a["dmax"], 0.5)
    _, o = flag(good_k)
    assert o[0].all(), "base points must be in view"
    _, o = flag(bad_k)
    assert not o[0].any(), "the far end must be rejected"
    while (np.abs(good_k - bad_k) > 1).any():
        mid = good_k + (bad_k - good_k) // 2
        mid = np.where(np.abs(good_k - bad_k) > 1, mid, good_k)
        _, o = flag(mid)
        inv = o[0].astype(bool)
        moved = np.abs(good_k - bad_k) > 1
        good_k = np.where(moved & inv, mid, good_k)
        bad_k = np.where(moved & ~inv, mid, bad_k)
    ga, go = flag(good_k)
    ba, bo = flag(bad_k)
    assert go[0].all() and not bo[0].any()
    # planted = the pair stands at THIS test's threshold: the in-view side's own output is within a few ulps of it
    u, v, cs = go[1].astype(np.float64), go[2].astype(np.float64), go[4].astype(np.float64)
    dist = np.linalg.norm(ga["P"].astype(np.float64) - Ow, axis=1)
    b = PLANT_BOUNDS.astype(np.float64)
    with np.errstate(all="ignore"):                  # dmin is 0 in the depth test
        near = {"z_behind": np.abs(ga["P"][:, 2].astype(np.float64) + float(PLANT_T[2])) < 1e-6,
                "u_below_minX": np.abs(u - b[0]) < 1e-3, "u_above_maxX": np.abs(u - b[1]) < 1e-3, "v_below_minY": np.abs(v - b[2]) < 1e-3, "v_above_maxY": np.abs(v - b[3]) < 1e-3,
                "dist_below_min": np.abs(dist / (0.8 * ga["dmin"].astype(np.float64)) - 1) < 1e-6,
                "dist_above_max": np.abs(dist / (1.2 * ga["dmax"].astype(np.float64)) - 1) < 1e-6, "cos_below_limit": np.abs(cs - 0.5) < 1e-6}[test]
    out = tuple(np.concatenate([ga[k], ba[k]]) for k in ("P", "Pn", "dmin", "dmax"))
    return out, near


# ---- vocabulary trees built by hand (the key layout of synth.make_vocabulary) ----------------------------------------------------------------------------
def _tree(children_of, seed):
    """children_of: {node: child count} in breadth-first numbering; nodes not named are leaves.  Node descriptors are random, children apart from their parent
    by a few bits so that descents spread."""
    rng = np.random.default_rng(seed)
    child_off, child_id, n_nodes = [0], [], 1
    node = 0
    parent = {0: None}
    while node < n_nodes:
        k = children_of.get(node, 0)
        for _ in range(k):
            parent[n_nodes] = node
            child_id.append(n_nodes); n_nodes += 1
        child_off.append(len(child_id))
        node += 1
    desc = np.zeros((n_nodes, 32), np.uint8)
    desc[0] = rng.integers(0, 256, 32, dtype=np.uint8)
    for i in range(1, n_nodes):
        bits = np.unpackbits(desc[parent[i]])
        desc[i] = np.packbits(bits ^ (rng.random(256) < 0.15))
    child_off = np.array(child_off, np.int32)
    leaf = np.diff(child_off) == 0
    word_id = -np.ones(n_nodes, np.int32); word_id[leaf] = np.arange(leaf.sum())
    weight = np.zeros(n_nodes); weight[leaf] = rng.uniform(0.5, 6.0, leaf.sum())
    depth = np.zeros(n_nodes, int)
    for i in range(1, n_nodes):
        depth[i] = depth[parent[i]] + 1
    return dict(n_nodes=n_nodes, L=int(depth.max()), child_off=child_off, child_id=np.array(child_id, np.int32), node_desc=desc, word_id=word_id, weight=weight), depth


TIE_FIRST, TIE_SECOND, SECOND_TRIP_NODE = 4, 71, 100      # node = child index + 1 under the root


def wide_vocabulary():
    """root with 130 children (three trips of 64); below it nodes with 1, 2, 63, 64 and 65 children; L = 3.  The root's children 3 and 70 (nodes TIE_FIRST and
    TIE_SECOND, in the first and the second trip) carry the same descriptor and both have children, so that a wrong winner also ends in a wrong word."""
    ch = {0: 130, 1: 1, 2: 2, 3: 63, TIE_FIRST: 64, 5: 65, TIE_SECOND: 63, 130: 65}
    ch[131] = 2                       # node 131, the only child of node 1, goes one level further: depth 3 exists; the rest of level 2 are leaves
    vocab, depth = _tree(ch, 61)
    vocab["node_desc"][TIE_SECOND] = vocab["node_desc"][TIE_FIRST]
    return vocab, depth


def ragged_vocabulary():
    """leaves at every depth 1..5: at each level the first child goes on and its siblings are leaves; fan-outs 3, 65, 2, 64, 130"""
    ch, node, n = {}, 0, 1
    for k in (3, 65, 2, 64, 130):
        ch[node] = k
        node, n = n, n + k            # the first child of this node is numbered n (breadth-first: the siblings are leaves and add nothing in between)
    vocab, depth = _tree(ch, 62)
    leaf_depths = set(depth[np.diff(vocab["child_off"]) == 0].tolist())
    assert leaf_depths == {1, 2, 3, 4, 5}, leaf_depths
    return vocab, depth


def bow_queries(vocab, n, seed):
    """n descriptors: noisy copies of random nodes' descriptors, some exact copies (distance 0), some random"""
    rng = np.random.default_rng(seed)
    src = vocab["node_desc"][rng.integers(1, vocab["n_nodes"], n)]
    bits = np.unpackbits(src, axis=1)
    d = np.packbits(bits ^ (rng.random(bits.shape) < 0.05), axis=1)
    d[::7] = src[::7]
    d[3::11] = rng.integers(0, 256, (len(d[3::11]), 32), dtype=np.uint8)
    return d
