"""Scenes shared by tests/test_fuse_sim3_cpu.py and tests/test_fuse_sim3_gpu.py (no test lives here).

scene_from_frames: the issue's scene.  Points of tests.test_ref_matcher._projected_case (2 500 points back-projected from frame 0's features); keyframes alternate
between the features of synth.gen_image(1000, 0) and gen_image(1000, 1), Sim3 scales cycle through 1.0, 1.7, 0.8, 1.2, "near" keyframes perturb the pose by
0.004 rad and 0.01 m, "far" ones by 0.08 rad and 0.25 m.

planted(): hand-made pairs with known answers.  The pose is the identity (Scw = [I | 0]: scw = 1, Rcw = I, tcw = 0, Ow = -0), fx = fy = 64, cx = 304, cy = 224 and the
points lie at depths that are powers of two, so u = 64 X / Z + 304 and v = 64 Y / Z + 224 are exact in f32 and dist3D = |P| is exact on the optical axis.
"""
import numpy as np

import tests.test_ref_matcher as trm
from ccm_slam_amd import fuse_sim3 as fs, synth

TH = 4.0
SCALES = (1.0, 1.7, 0.8, 1.2)


def frame_features(frames):
    """[(xy, octave, desc)] of the two extracted frames"""
    return [(np.stack([k["x"], k["y"]], 1).astype(np.float32), k["octave"].astype(np.uint8), np.ascontiguousarray(d)) for k, d in frames]


def scene_from_frames(frames, kinds, seed=8, n_pts=None, first=0):
    """kinds: a string of 'n' (near) and 'f' (far), one per keyframe; points first .. first + n_pts.  Returns (Scene, the _projected_case dict, S16 (K, 16) for the reference, which frame each shows)"""
    s = trm._projected_case(frames, seed)
    rng = np.random.default_rng(1000 + seed)
    Scw = np.stack([fs.perturbed_scw(rng, SCALES[k % 4], *((0.004, 0.01) if c == "n" else (0.08, 0.25))) for k, c in enumerate(kinds)])
    which = [k % 2 for k in range(len(kinds))]
    p = slice(first, s["n_pts"] if n_pts is None else first + n_pts)      # (the scene's first 40 points lie behind the camera)
    sc = fs.assemble(frame_features(frames), which, Scw, s["K4"], s["sf"], TH, s["Xw"][p], s["normal"][p], s["dmin"][p], s["dmax"][p], s["pdesc"][p], trm.BOUNDS)
    S16 = np.zeros((len(kinds), 16), np.float32); S16[:, :12] = Scw; S16[:, 15] = 1
    return sc, s, S16, which


def ref_fuse(rlib, frames, s, S16, which, k, pdesc=None):
    """the reference's own ORBmatcher::Fuse(pKF, Scw, ...) for keyframe k with kf_has_mp all zero: (nFused, best_idx, valid, u, v, level)"""
    import ctypes as C
    kps, desc = frames[which[k]]
    c, _p = trm.c, trm._p
    n = s["n_pts"]
    best = np.zeros(n, np.int32); valid, u, v, lvl = trm._proj_out(n)
    has = np.zeros(len(kps), np.uint8)
    pd = s["pdesc"] if pdesc is None else np.ascontiguousarray(pdesc, np.uint8)
    rlib.ref_fuse_sim3.restype = C.c_int
    nf = rlib.ref_fuse_sim3(_p(c(kps["x"])), _p(c(kps["y"])), _p(c(kps["octave"])), _p(desc), len(kps), *trm.fb, _p(s["sf"]), _p(s["isig"]), _p(s["K4"]), _p(c(S16[k])),
                            _p(has), n, _p(s["Xw"]), _p(s["normal"]), _p(s["dmin"]), _p(s["dmax"]), _p(pd), C.c_float(TH), _p(best), _p(valid), _p(u), _p(v), _p(lvl))
    return nf, best, valid, u, v, lvl


def assert_reference_scene(refs, kinds):
    """what the issue asserts on the reference alone before anything is compared with it"""
    hits = [r[0] for r in refs]; valids = [int(r[2].sum()) for r in refs]
    assert all(h >= 900 for h, c in zip(hits, kinds) if c == "n"), hits
    assert len({v for v, c in zip(valids, kinds) if c == "f"}) >= 3, valids
    assert len(set(hits)) >= 2, hits


def same_as_reference(t, uv, ref, tag):
    """one keyframe's row of the unpacked table against what ref_fuse returned; every comparison is exact"""
    nf, best, valid, u, v, lvl = ref
    m = valid > 0
    assert np.array_equal(t["status"] >= 4, m), tag
    if uv is not None:
        assert np.array_equal(uv[m, 0].view(np.uint32), u[m].view(np.uint32)) and np.array_equal(uv[m, 1].view(np.uint32), v[m].view(np.uint32)), tag
    assert np.array_equal(t["level"][m], lvl[m]), tag
    hit = t["status"] == 7
    assert np.array_equal(hit, best >= 0), tag
    assert np.array_equal(t["idx"][hit], best[hit]), tag
    assert int(hit.sum()) == nf, tag


# ---------------------------------------------------------------------------------------------------------------------------------------------
# planted pairs
# ---------------------------------------------------------------------------------------------------------------------------------------------
K4 = np.array([64.0, 64.0, 304.0, 224.0], np.float32)
IDENT = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
f32 = np.float32


def _flip(desc, nbits):
    d = np.unpackbits(np.asarray(desc, np.uint8)).copy()
    d[:nbits] ^= 1
    return np.packbits(d)


class Planted:
    """K keyframes with hand-made features and grids, P points; expect[(k, i)] = (status, idx or None, dist or None, level or None)"""

    def __init__(self, nlevels=8):
        self.sf = synth.scale_tables(nlevels)[0]
        self.kfs = []      # (xy (n, 2), oct, desc (n, 32), Scw12, (cell_off, cell_idx) or None)
        self.pts = []      # (pos, normal, dmin, dmax, desc)
        self.expect = {}

    def kf(self, feats=(), Scw=IDENT, grid=None):
        xy = np.array([f[0] for f in feats], np.float32).reshape(-1, 2)
        oc = np.array([f[1] for f in feats], np.uint8)
        de = np.array([f[2] for f in feats], np.uint8).reshape(-1, 32)
        self.kfs.append((xy, oc, de, np.asarray(Scw, np.float32), grid))
        return len(self.kfs) - 1

    def pt(self, pos, normal=None, dmin=1e-3, dmax=None, desc=None):
        pos = np.asarray(pos, np.float32)
        with np.errstate(all="ignore"):
            d = float(np.linalg.norm(pos.astype(np.float64)))
            n = pos / f32(d) if normal is None else np.asarray(normal, np.float32)
        self.pts.append((pos, n, f32(dmin), f32(d if dmax is None else dmax), np.zeros(32, np.uint8) if desc is None else np.asarray(desc, np.uint8)))
        return len(self.pts) - 1

    def scene(self):
        off = [0]; xy = []; oc = []; de = []; co = []; ci = []; rec = []; S = []
        for kxy, koc, kde, Scw, grid in self.kfs:
            g = fs.build_grid(kxy, trm.BOUNDS) if grid is None else grid
            off.append(off[-1] + len(koc)); xy.append(kxy.reshape(-1)); oc.append(koc); de.append(kde.reshape(-1)); co.append(np.asarray(g[0], np.int32))
            ci.append(np.asarray(g[1], np.int32)); rec.append(fs.kf_record(K4, trm.BOUNDS)); S.append(Scw)
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
        p = self.pts
        return fs.Scene(cat(rec, np.float32), off, cat(xy, np.float32), cat(oc, np.uint8), cat(de, np.uint8), cat(co, np.int32), cat(ci, np.int32), cat(S, np.float32),
                        self.sf, fs.log_scale_factor(self.sf), TH, np.array([q[0] for q in p], np.float32), np.array([q[1] for q in p], np.float32),
                        np.array([q[2] for q in p], np.float32), np.array([q[3] for q in p], np.float32), np.array([q[4] for q in p], np.uint8))

    def check(self, table, tag=""):
        t = fs.unpack_table(table)
        for (k, i), (st, idx, dist, lvl) in self.expect.items():
            got = (int(t["status"][k, i]), int(t["idx"][k, i]), int(t["dist"][k, i]), int(t["level"][k, i]))
            assert got[0] == st, (tag, k, i, got, st)
            if idx is not None:
                assert got[1] == idx, (tag, k, i, got, idx)
            if dist is not None:
                assert got[2] == dist, (tag, k, i, got, dist)
            if lvl is not None:
                assert got[3] == lvl, (tag, k, i, got, lvl)


def on_axis(z):
    """a point on the optical axis at depth z: u = cx, v = cy, dist3D = z"""
    return (0.0, 0.0, z)


def planted():
    """Every boundary the issue names, in one scene.  Keyframe 0 has no features (every pair that passes the gates ends as status 4)."""
    rng = np.random.default_rng(5)
    q = rng.integers(0, 256, 32, dtype=np.uint8)
    pl = Planted()
    E = pl.expect
    k0 = pl.kf()
    # z == 0: invz = inf, x = 0 * inf = NaN or X * inf = inf: outside the image, not behind the camera
    E[k0, pl.pt((0, 0, 0), normal=(0, 0, 1), dmax=1)] = (1, -1, -1, None)
    E[k0, pl.pt((1, 0, 0), dmax=1)] = (1, -1, -1, None)
    E[k0, pl.pt((0, 0, -1), dmax=1)] = (0, -1, -1, None)
    # the image bounds at depth 4: u = 16 X + 304, v = 16 Y + 224; >= min and < max on the int bounds 0, 0, 752, 480
    # (the floats just below the lower bounds give u = -2^-15 and v = -2^-16 exactly; just below the upper bounds the sum would round back onto the bound)
    for pos, st in (((-19, 0, 4), 4), ((28, 0, 4), 1), ((0, -14, 4), 4), ((0, 16, 4), 1), ((np.nextafter(f32(-19), f32(-20)), 0, 4), 1),
                    ((27.5, 0, 4), 4), ((0, np.nextafter(f32(-14), f32(-15)), 4), 1), ((0, 15.5, 4), 4)):
        E[k0, pl.pt(pos, dmax=64)] = (st, -1, -1, None)
    # the distance range: dist3D exactly 0.8f * dmin and 1.2f * dmax are inside, their outer neighbours are not
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
    # an all-zero Scw: scw = 0, Rcw = 0 * inf = NaN: outside the image for every point
    kz = pl.kf(Scw=np.zeros(12, np.float32))
    for i in range(len(pl.pts)):
        E[kz, i] = (1, -1, -1, None)
    # the Hamming threshold: one feature under the projection (304, 224) of an on-axis point, 50 and 51 bits away
    i_q0 = pl.pt(on_axis(4), dmax=4, desc=q)                        # level 0
    i_q3 = pl.pt(on_axis(4), dmax=4 * 1.2 ** 2.5, desc=q)            # level 3
    i_q7 = pl.pt(on_axis(4), dmax=4000, desc=q)                      # level 7
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
    # the window's edge: r = 4 at level 0; |dx| < r, so a feature 4 px away is not in the window and one just inside is
    k = pl.kf([((308.0, 224.0), 0, q), ((304.0, 220.0), 0, q)])
    E[k, i_q0] = (4, -1, -1, 0)
    k = pl.kf([((np.nextafter(f32(308), f32(0)), 224.0), 0, _flip(q, 7))])
    E[k, i_q0] = (7, 0, 7, 0)
    # ties.  Equal descriptors on two features of ONE cell, the lower feature index later in the cell: the earlier position wins
    feats = [((100.0, 100.0), 0, _flip(q, 200)), ((303.0, 224.0), 0, _flip(q, 9)), ((20.0, 20.0), 0, _flip(q, 200)), ((305.0, 224.0), 0, _flip(q, 9))]
    xy = np.array([f[0] for f in feats], np.float32)
    off, idx = fs.build_grid(xy, trm.BOUNDS)
    cell = lambda x, y: int(round(x * 75 / 752)) * 48 + int(round(y * 48 / 480))
    c = cell(304, 224)
    assert off[c + 1] - off[c] == 2 and list(idx[off[c]:off[c + 1]]) == [1, 3]
    swapped = idx.copy(); swapped[off[c]:off[c + 1]] = [3, 1]
    E[pl.kf(feats), i_q0] = (7, 1, 9, 0)
    E[pl.kf(feats, grid=(off, swapped)), i_q0] = (7, 3, 9, 0)
    # ... and in TWO cells: feature 3 in the cell of the lower ix comes first in the traversal, feature 1 in the next column second
    feats2 = [((100.0, 100.0), 0, _flip(q, 200)), ((307.0, 224.0), 0, _flip(q, 9)), ((20.0, 20.0), 0, _flip(q, 200)), ((301.0, 224.0), 0, _flip(q, 9))]
    assert cell(307, 224) == cell(301, 224) + 48
    E[pl.kf(feats2), i_q0] = (7, 3, 9, 0)
    # a strictly better candidate later in the traversal still wins
    feats3 = [((301.0, 224.0), 0, _flip(q, 9)), ((307.0, 224.0), 0, _flip(q, 8))]
    E[pl.kf(feats3), i_q0] = (7, 1, 8, 0)
    return pl


DISC_SIZES = (0, 1, 60, 64, 65, 70, 300)


def disc():
    """Keyframes with DISC_SIZES features inside a 6 px disc around (304, 224), all octaves, so that the cells a window reads hold that many: up to 64 a lane walks the
    window alone, beyond that the wave takes it.  Queries on the optical axis at every predicted level (r = 4 * 1.2^level: the level-7 window holds the whole disc)
    and off the axis at level 0 (the 8 x 8 px window holds a part of it)."""
    rng = np.random.default_rng(11)
    q = rng.integers(0, 256, 32, dtype=np.uint8)
    pl = Planted()
    for n in DISC_SIZES:
        a = rng.uniform(0, 2 * np.pi, n); rad = 6 * np.sqrt(rng.uniform(0, 1, n))
        pl.kf([((304 + rad[j] * np.cos(a[j]), 224 + rad[j] * np.sin(a[j])), j % 8, _flip(rng.permutation(q) if j % 3 else q, int(rng.integers(0, 120)))) for j in range(n)])
    for lvl in range(8):
        pl.pt(on_axis(4), dmax=4 * 1.2 ** (lvl - 0.5) if lvl else 4, desc=q)
    for dx in (-5.0, -3.0, 2.0, 6.0, 9.0):
        pl.pt((dx / 16, 0, 4), dmax=float(np.linalg.norm([dx / 16, 0, 4])), desc=q)
    return pl
