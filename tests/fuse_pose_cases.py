"""Scenes shared by tests/test_fuse_pose_cpu.py and tests/test_fuse_pose_gpu.py (no test lives here).

fan_out_scene: the issue's scene.  Nine keyframes that all show frame 0's features: 0 .. 7 at the eight poses of tests.test_ref_matcher._fuse_fan_out_case, 8 (the
CURRENT keyframe of the mirror tests) at the pose of _projected_case.  7 500 points: the 2 500 of _projected_case(frames, 7) (the current keyframe's points), the
2 500 of _fuse_fan_out_case (the pool the fuse candidates of the second direction are taken from) and the 2 500 of _projected_case(frames, 8), which only make the
scene large enough for a job of 6 000 points.  Ow of every keyframe comes from the project's restatement of
KeyFrame::SetPose (fuse_pose.pose_record -> sim3_correct.camera_center, the lines of csrc/gba_apply_math.h); ref_fuse builds its own.

planted(): hand-made pairs with known answers.  The pose is the identity, fx = fy = 1, cx = cy = 0, and the points lie at depth 1 (u = X, v = Y exactly) or on the
optical axis (u = v = 0, dist3D = Z exactly).
"""
import ctypes as C

import numpy as np

import oracle
import tests.test_ref_matcher as trm
from ccm_slam_amd import fuse_pose as fp, fuse_sim3 as fs, synth
from fuse_sim3_cases import Planted, _flip, frame_features, on_axis

f32 = np.float32
CALLS = [0, 1, 5, 6, 1, 5, 2, 7, 3, 3, 4, 6]      # the target of every Fuse call of the fan-out, pinned by tests/test_ref_matcher.py
CURRENT = 8
N_KF = 9


def fan_out_scene(frames, th=fp.TH):
    """(Scene without jobs, info) with info = dict(s7, s17, T16 (9, 16), n1 = 2 500 points of the current keyframe, n2 = 2 500 pool points)"""
    s8 = trm._projected_case(frames, 8)
    s7 = trm._projected_case(frames, 7)
    s17, Ts, _, nb1, nb2 = trm._fuse_fan_out_case(frames)
    T16 = np.concatenate([Ts.reshape(8, 16), s7["T"].reshape(1, 16)]).astype(np.float32)
    cat = lambda k: np.concatenate([s7[k], s17[k], s8[k]])
    sc = fp.assemble(frame_features(frames)[:1], [0] * N_KF, T16, s7["K4"], s7["sf"], s7["isig"], th, cat("Xw"), cat("normal"), cat("dmin"), cat("dmax"), cat("pdesc"),
                     (), trm.BOUNDS)
    return sc, dict(s7=s7, s17=s17, T16=np.ascontiguousarray(T16), n1=s7["n_pts"], n2=s17["n_pts"])


def all_pairs_jobs(K, P, first=0):
    return [(k, first, P) for k in range(K)]


def ref_fuse(rlib, frames, sc, info, k, pts=None, pdesc=None, th=None):
    """the reference's own ORBmatcher::Fuse(pKF, vpMapPoints, th) for keyframe k with kf_has_mp all zero on the points `pts` (indices; None: the current keyframe's
    2 500), optionally with other descriptors for them: (nFused, best_idx, valid, u, v, level)"""
    kps, desc = frames[0]
    c, _p = trm.c, trm._p
    pts = np.arange(info["n1"]) if pts is None else np.asarray(pts)
    n = int(pts.size)
    take = lambda a, w: np.ascontiguousarray(a.reshape(-1, w)[pts])
    best = np.zeros(n, np.int32); valid, u, v, lvl = trm._proj_out(n)
    has = np.zeros(len(kps), np.uint8)
    pd = take(sc.pt_desc, 32) if pdesc is None else np.ascontiguousarray(pdesc, np.uint8)
    s = info["s7"]
    rlib.ref_fuse.restype = C.c_int
    nf = rlib.ref_fuse(_p(c(kps["x"])), _p(c(kps["y"])), _p(c(kps["octave"])), _p(desc), len(kps), *trm.fb, _p(s["sf"]), _p(s["isig"]), _p(s["K4"]), _p(c(info["T16"][k])),
                       _p(has), n, _p(take(sc.pos, 3)), _p(take(sc.normal, 3)), _p(take(sc.min_dist, 1)), _p(take(sc.max_dist, 1)), _p(pd),
                       C.c_float(sc.th if th is None else th), _p(best), _p(valid), _p(u), _p(v), _p(lvl))
    return nf, best, valid, u, v, lvl


def assert_reference_scene(refs, frames, info, th):
    """what the issue asserts on the reference alone before anything is compared with it; refs[k] = ref_fuse of keyframe k on the current keyframe's points.
    The bounds are those of tests/test_ref_matcher.py (test_fuse_M7_chi2_gate, test_fuse_fan_out_of_search_in_neighbors_M7_xS)."""
    s = info["s7"]; kps = s["kps"]
    nf, best, valid, u, v, lvl = refs[CURRENT]
    assert 1500 < valid.sum() < s["n_pts"] - 100
    if th == 3.0:
        assert nf > 800
    hits = [r[0] for r in refs[:8]]
    assert all(h > 100 for h in hits), hits
    assert len(set(hits)) >= 3, hits
    on, _, _, _ = oracle.projected_window_search(kps["x"], kps["y"], kps["octave"], s["desc"], trm.BOUNDS, s["sf"], s["isig"], valid, u, v, lvl, s["pdesc"], th, True, 50)
    off, _, _, _ = oracle.projected_window_search(kps["x"], kps["y"], kps["octave"], s["desc"], trm.BOUNDS, s["sf"], s["isig"], valid, u, v, lvl, s["pdesc"], th, False, 50)
    assert on == nf and off > on      # the chi-square gate matters here


def e2_of(u, v, kpx, kpy):
    """e2 of ORBmatcher.cpp:946-948 on plain numpy f32: two products and one sum, each rounded to f32"""
    ex = f32(u) - np.asarray(kpx, f32); ey = f32(v) - np.asarray(kpy, f32)
    return ((ex * ex).astype(f32) + (ey * ey).astype(f32)).astype(f32)


def chi2(u, v, kpx, kpy, inv_sigma2):
    """e2 * mvInvLevelSigma2[kpLevel] of :950: one more f32 product (compared as a double against 5.99)"""
    return (e2_of(u, v, kpx, kpy) * np.asarray(inv_sigma2, f32)).astype(f32)


def passes(g):
    return np.asarray(g, f32).astype(np.float64) <= 5.99


G_PASS = np.nextafter(f32(5.99), f32(0)) if float(f32(5.99)) > 5.99 else f32(5.99)      # the largest float that is not > 5.99
G_FAIL = np.nextafter(G_PASS, f32(9))


def e2_boundary(inv_sigma2):
    """(a, b): neighbouring floats of e2 with a * invSigma2 the largest product that is not > 5.99 and b = the next float up, whose product is"""
    isig = f32(inv_sigma2)
    a = f32(5.99 / float(isig))
    while passes(f32(np.nextafter(a, f32(1e9)) * isig)):
        a = np.nextafter(a, f32(1e9))
    while not passes(f32(a * isig)):
        a = np.nextafter(a, f32(0))
    b = np.nextafter(a, f32(1e9))
    assert passes(f32(a * isig)) and not passes(f32(b * isig))
    return a, b


def chi2_boundary(u, v, want_e2):
    """a feature position (kpx, kpy) whose e2_of() from (u, v) is exactly the float want_e2, found by searching neighbouring floats around ey = 0.47 (kpy < 1, where
    the floats are dense enough for every float of e2 to be reachable)"""
    ey = 0.47
    ex = np.sqrt(float(want_e2) - ey * ey)
    kx0 = f32(u - ex); ky0 = f32(v + ey)
    kxs = [kx0]; kys = [ky0]
    for _ in range(40):
        kxs.append(np.nextafter(kxs[-1], f32(1e9)))
    a = ky0; b = ky0
    for _ in range(400):
        a = np.nextafter(a, f32(-1e9)); b = np.nextafter(b, f32(1e9)); kys += [a, b]
    KX, KY = np.meshgrid(np.array(kxs, f32), np.array(kys, f32))
    hit = np.argwhere(e2_of(u, v, KX, KY).view(np.uint32) == f32(want_e2).view(np.uint32))
    assert hit.size, (u, v, want_e2)
    i, j = hit[0]
    return float(KX[i, j]), float(KY[i, j])


K4 = np.array([1.0, 1.0, 0.0, 0.0], f32)
IDENT = np.eye(4, dtype=f32).reshape(16)


def at(u, v):
    """a point at depth 1 that projects to (u, v) exactly"""
    return (u, v, 1.0)


class PlantedPose(Planted):
    """fuse_sim3_cases.Planted for ccm_fuse_pose_eval: identity pose, fx = fy = 1, cx = cy = 0; one job per keyframe over all points, so that the table reads as
    (K, P) and Planted.check applies.  expect[(k, i)] = (status, idx or None, dist or None, level or None)"""

    def scene(self, inv_sigma2=None, th=fp.TH):
        off = [0]; xy = []; oc = []; de = []; co = []; ci = []; rec = []
        for kxy, koc, kde, _, grid in self.kfs:
            g = fs.build_grid(kxy, trm.BOUNDS) if grid is None else grid
            off.append(off[-1] + len(koc)); xy.append(kxy.reshape(-1)); oc.append(koc); de.append(kde.reshape(-1)); co.append(np.asarray(g[0], np.int32))
            ci.append(np.asarray(g[1], np.int32)); rec.append(fs.kf_record(K4, trm.BOUNDS))
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
        p = self.pts
        K = len(self.kfs)
        isig = synth.scale_tables(len(self.sf))[3] if inv_sigma2 is None else np.asarray(inv_sigma2, f32)
        return fp.Scene(cat(rec, f32), off, cat(xy, f32), cat(oc, np.uint8), cat(de, np.uint8), cat(co, np.int32), cat(ci, np.int32), fp.pose_record(np.tile(IDENT, (K, 1))),
                        self.sf, isig, fs.log_scale_factor(self.sf), th, np.array([q[0] for q in p], f32), np.array([q[1] for q in p], f32),
                        np.array([q[2] for q in p], f32), np.array([q[3] for q in p], f32), np.array([q[4] for q in p], np.uint8), all_pairs_jobs(K, len(p)))

    def check(self, table, tag=""):
        super().check(np.asarray(table).reshape(len(self.kfs), len(self.pts)), tag)


def planted():
    """Every boundary the issue names, in one scene.  Keyframe 0 has no features (every pair that passes the gates ends as status 4).  th = 3: r = 3 at level 0."""
    rng = np.random.default_rng(5)
    q = rng.integers(0, 256, 32, dtype=np.uint8)
    sf, _, _, isig = synth.scale_tables()
    pl = PlantedPose()
    E = pl.expect
    k0 = pl.kf()
    # z == 0: invz = inf, x = 0 * inf = NaN or X * inf = inf: outside the image, not behind the camera
    E[k0, pl.pt((0, 0, 0), normal=(0, 0, 1), dmax=1)] = (1, -1, -1, None)
    E[k0, pl.pt((1, 0, 0), dmax=1)] = (1, -1, -1, None)
    E[k0, pl.pt((0, 0, -1), dmax=1)] = (0, -1, -1, None)
    # the image bounds at depth 1: u = X, v = Y; >= min and < max on the int bounds 0, 0, 752, 480
    tiny = f32(-2.0 ** -100)      # a normal float just below the bound
    for pos, st in ((at(0, 10), 4), (at(752, 10), 1), (at(10, 0), 4), (at(10, 480), 1), (at(tiny, 10), 1), (at(np.nextafter(f32(752), f32(0)), 10), 4), (at(10, tiny), 1),
                    (at(10, np.nextafter(f32(480), f32(0))), 4)):
        E[k0, pl.pt(pos)] = (st, -1, -1, None)
    # the distance range: dist3D exactly 0.8f * dmin and 1.2f * dmax are inside, their outer neighbours are not (on the axis: u = v = 0, inside the image)
    lo = f32(0.8) * f32(5.0); hi = f32(1.2) * f32(5.0)
    for z, st, kw in ((lo, 4, dict(dmin=5.0, dmax=50.0)), (np.nextafter(lo, f32(0)), 2, dict(dmin=5.0, dmax=50.0)), (np.nextafter(lo, f32(9)), 4, dict(dmin=5.0, dmax=50.0)),
                      (hi, 4, dict(dmin=0.1, dmax=5.0)), (np.nextafter(hi, f32(9)), 2, dict(dmin=0.1, dmax=5.0)), (np.nextafter(hi, f32(0)), 4, dict(dmin=0.1, dmax=5.0))):
        E[k0, pl.pt(on_axis(z), normal=(0, 0, 1), **kw)] = (st, -1, -1, None)
    # the viewing angle: PO . Pn == 0.5 dist3D passes, the next float below fails
    E[k0, pl.pt(on_axis(4), normal=(0, 0, 0.5), dmax=4)] = (4, -1, -1, 0)
    E[k0, pl.pt(on_axis(4), normal=(0, 0, np.nextafter(f32(0.5), f32(0))), dmax=4)] = (3, -1, -1, None)
    # the predicted level: ratio 1 -> ceil(0) = 0; a huge ratio -> nlevels - 1; a ratio below 1 -> clamped to 0
    E[k0, pl.pt(on_axis(4), dmax=4)] = (4, -1, -1, 0)
    E[k0, pl.pt(on_axis(4), dmax=4000)] = (4, -1, -1, 7)
    E[k0, pl.pt(on_axis(4), dmax=3.5)] = (4, -1, -1, 0)
    # NaN and Inf positions
    E[k0, pl.pt((np.nan, 0, 4), normal=(0, 0, 1), dmax=4)] = (1, -1, -1, None)
    E[k0, pl.pt((0, 0, np.nan), normal=(0, 0, 1), dmax=4)] = (1, -1, -1, None)
    E[k0, pl.pt((0, 0, np.inf), normal=(0, 0, 1), dmax=4)] = (1, -1, -1, None)
    E[k0, pl.pt((0, 0, -np.inf), normal=(0, 0, 1), dmax=4)] = (0, -1, -1, None)
    E[k0, pl.pt((np.inf, 0, 4), normal=(0, 0, 1), dmax=4)] = (1, -1, -1, None)
    # queries at (304, 224): dist3D = sqrt(304^2 + 224^2 + 1) is pt()'s own f32 norm, so dmax = that norm gives ratio 1 and level 0
    d = float(np.linalg.norm([304.0, 224.0, 1.0]))
    i_q0 = pl.pt(at(304, 224), desc=q)                               # level 0
    i_q3 = pl.pt(at(304, 224), dmax=d * 1.2 ** 2.5, desc=q)          # level 3
    i_q7 = pl.pt(at(304, 224), dmax=d * 1000, desc=q)                # level 7
    E[k0, i_q0] = (4, -1, -1, 0); E[k0, i_q3] = (4, -1, -1, 3); E[k0, i_q7] = (4, -1, -1, 7)
    # the Hamming threshold: one feature under the projection, 0, 50, 51 and 256 bits away (256: reported as far, with its index)
    for nb, st in ((0, 7), (50, 7), (51, 6), (256, 6)):
        k = pl.kf([((304.0, 224.0), 0, _flip(q, nb))])
        E[k, i_q0] = (st, 0, nb, 0)
        E[k, i_q3] = (5, -1, -1, 3)                                  # octave 0 is no candidate at level 3
    # the level filter: octaves level - 2 .. level + 1 at level 3; at level 0 only octave 0; at level 7 octaves 6 and 7
    for o, st3, st0, st7 in ((0, 5, 7, 5), (1, 5, 5, 5), (2, 7, 5, 5), (3, 7, 5, 5), (4, 5, 5, 5), (6, 5, 5, 7), (7, 5, 5, 7)):
        k = pl.kf([((304.0, 224.0), o, _flip(q, 3))])
        E[k, i_q3] = (st3, 0 if st3 == 7 else -1, 3 if st3 == 7 else -1, 3)
        E[k, i_q0] = (st0, 0 if st0 == 7 else -1, 3 if st0 == 7 else -1, 0)
        E[k, i_q7] = (st7, 0 if st7 == 7 else -1, 3 if st7 == 7 else -1, 7)
    # the window's edge: r = 3 at level 0; |dx| < r, so a feature 3 px away is not in the window; one just inside is, but it lies outside the chi-square circle
    # (sqrt(5.99) = 2.447 px at level 0), so the window is not empty and nobody passes
    k = pl.kf([((307.0, 224.0), 0, q), ((304.0, 221.0), 0, q)])
    E[k, i_q0] = (4, -1, -1, 0)
    k = pl.kf([((np.nextafter(f32(307), f32(0)), 224.0), 0, q)])
    E[k, i_q0] = (5, -1, -1, 0)
    # inside the window's box, outside the circle, and the nearest descriptor: it must not win
    k = pl.kf([((306.2, 226.2), 0, q), ((305.0, 224.0), 0, _flip(q, 9))])
    E[k, i_q0] = (7, 1, 9, 0)
    pl.k_box = k; pl.i_q0 = i_q0
    # the chi-square boundary at level 0 (invSigma2 = 1) and at level 1 (invSigma2 = 1 / 1.44): queries at (8, 0.5), where neighbouring floats are dense enough
    # for every float of e2 to be reachable
    dq = float(np.linalg.norm([8.0, 0.5, 1.0]))
    for lvl, dmax in ((0, None), (1, dq * 1.2 ** 0.5)):
        iq = pl.pt(at(8, 0.5), dmax=dmax, desc=q)
        E[k0, iq] = (4, -1, -1, lvl)
        lo, hi = e2_boundary(isig[lvl])
        if lvl == 0:
            assert lo == G_PASS and hi == G_FAIL
        for want, st in ((lo, 7), (hi, 5)):
            kx, ky = chi2_boundary(8.0, 0.5, want)
            g = chi2(8.0, 0.5, kx, ky, isig[lvl])
            assert e2_of(8.0, 0.5, kx, ky) == want and bool(passes(g)) == (st == 7)          # on plain numpy f32 first
            assert abs(kx - 8.0) < 3.0 * sf[lvl] and abs(ky - 0.5) < 3.0 * sf[lvl]          # in the window
            k = pl.kf([((kx, ky), lvl, q)])
            E[k, iq] = (st, 0 if st == 7 else -1, 0 if st == 7 else -1, lvl)
    # ties.  Equal descriptors on two features of ONE cell, the lower feature index later in the cell: the earlier position wins
    feats = [((100.0, 100.0), 0, _flip(q, 200)), ((303.0, 224.0), 0, _flip(q, 9)), ((20.0, 20.0), 0, _flip(q, 200)), ((305.0, 224.0), 0, _flip(q, 9))]
    xy = np.array([f[0] for f in feats], f32)
    off, idx = fs.build_grid(xy, trm.BOUNDS)
    cell = lambda x, y: int(round(x * 75 / 752)) * 48 + int(round(y * 48 / 480))
    c = cell(304, 224)
    assert off[c + 1] - off[c] == 2 and list(idx[off[c]:off[c + 1]]) == [1, 3]
    swapped = idx.copy(); swapped[off[c]:off[c + 1]] = [3, 1]
    E[pl.kf(feats), i_q0] = (7, 1, 9, 0)
    E[pl.kf(feats, grid=(off, swapped)), i_q0] = (7, 3, 9, 0)
    # ... and in TWO cells: feature 3 in the cell of the lower ix comes first in the traversal, feature 1 in the next column second
    feats2 = [((100.0, 100.0), 0, _flip(q, 200)), ((306.0, 224.0), 0, _flip(q, 9)), ((20.0, 20.0), 0, _flip(q, 200)), ((302.0, 224.0), 0, _flip(q, 9))]
    assert cell(306, 224) == cell(302, 224) + 48
    E[pl.kf(feats2), i_q0] = (7, 3, 9, 0)
    # a strictly better candidate later in the traversal still wins
    feats3 = [((302.0, 224.0), 0, _flip(q, 9)), ((306.0, 224.0), 0, _flip(q, 8))]
    E[pl.kf(feats3), i_q0] = (7, 1, 8, 0)
    return pl


DISC_SIZES = (0, 1, 60, 64, 65, 70, 300)
DISC_WHOLE = 4       # from this predicted level on the window's box (r = 3 * 1.2^level >= 6.2 px) holds the whole 6 px disc


def disc():
    """Keyframes with DISC_SIZES features inside a 6 px disc around (304, 224), all octaves, so that the cells a window reads hold that many: up to 64 a lane walks the
    window alone, beyond that the wave takes it.  Points 0 .. 7: queries at (304, 224) at every predicted level; then queries off the centre at level 0."""
    rng = np.random.default_rng(11)
    q = rng.integers(0, 256, 32, dtype=np.uint8)
    pl = PlantedPose()
    for n in DISC_SIZES:
        a = rng.uniform(0, 2 * np.pi, n); rad = 6 * np.sqrt(rng.uniform(0, 1, n))
        pl.kf([((304 + rad[j] * np.cos(a[j]), 224 + rad[j] * np.sin(a[j])), j % 8, _flip(rng.permutation(q) if j % 3 else q, int(rng.integers(0, 120)))) for j in range(n)])
    d = float(np.linalg.norm([304.0, 224.0, 1.0]))
    for lvl in range(8):
        pl.pt(at(304, 224), dmax=d * 1.2 ** (lvl - 0.5) if lvl else None, desc=q)
    for dx in (-5.0, -3.0, 2.0, 6.0, 9.0):
        pl.pt(at(304 + dx, 224), desc=q)
    return pl


def disc_gate_counts(pl, k, lvl):
    """(passing, failing) candidates of keyframe k at the level filter of predicted level lvl under the chi-square gate, for the query at (304, 224)"""
    kxy, koc = pl.kfs[k][0], pl.kfs[k][1].astype(int)
    isig = synth.scale_tables()[3]
    at_level = (koc >= lvl - 1) & (koc <= lvl)
    g = chi2(304.0, 224.0, kxy[:, 0], kxy[:, 1], isig[np.minimum(koc, 7)]) if len(koc) else np.zeros(0, f32)
    ok = g.astype(np.float64) <= 5.99
    return int((at_level & ok).sum()), int((at_level & ~ok).sum())
