"""Scenes shared by tests/test_sim3_search_cpu.py and tests/test_sim3_search_gpu.py (no test lives here).

projection_case / pair_case: the set-ups of tests.test_ref_matcher.test_search_by_projection_sim3_M9_claims and test_search_by_sim3_M10, copied, so that the
reference's own ORBmatcher.cpp runs on them through the driver entries ref_search_by_projection_sim3 and ref_search_by_sim3.

PairPlanted: hand-made pairs of the SearchBySim3 gate with known answers.  As in fuse_sim3_cases.planted() the source pose and the transform are the identity unless a
case says otherwise, fx = fy = 64, cx = 304, cy = 224, and the depths are powers of two, so u = 64 X / Z + 304 and v = 64 Y / Z + 224 are exact in f32.
"""
import ctypes as C

import numpy as np

import tests.test_ref_matcher as trm
from ccm_slam_amd import fuse_sim3 as fs, sim3_search as ss, synth
from fuse_sim3_cases import K4, Planted, _flip, frame_features, on_axis

f32 = np.float32
c, _p = trm.c, trm._p
IDENT12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)      # R (9), t (3)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the projection scene (M9)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def projection_case(frames):
    """2 500 points, 120 draws of features matched on entry, 150 points the keyframe observes already"""
    s = trm._projected_case(frames, 9, sim3_scale=0.8)
    N = s["N"]
    rng = s["rng"]
    matched0 = -np.ones(N, np.int32); matched0[rng.integers(0, N, 120)] = 1_000_000
    existing = -np.ones(s["n_pts"], np.int32)
    already = rng.choice(s["n_pts"], 150, replace=False)
    free = np.flatnonzero(matched0 < 0)
    existing[already] = rng.choice(free, 150, replace=False)
    return dict(s=s, matched0=matched0, existing=existing, no_claim=(existing >= 0).astype(np.uint8))


def projection_scene(frames, case, th) -> fs.Scene:
    """the case as a one-keyframe fuse_sim3.Scene with the caller's grid (the reference's candidate order)"""
    s = case["s"]
    xy, oc, de = frame_features(frames)[0]
    return ss.single_keyframe_scene(xy, oc, de, s["K4"], trm.BOUNDS, s["S"][:3, :].reshape(-1), s["sf"], float(th), s["Xw"], s["normal"], s["dmin"], s["dmax"], s["pdesc"])


def ref_projection(rlib, case, th):
    """the reference's own SearchByProjection(pKF, Scw, ...): (n, matched on exit, valid, u, v, level)"""
    s = case["s"]; kps = s["kps"]; N = s["N"]
    got = case["matched0"].copy(); valid, u, v, lvl = trm._proj_out(s["n_pts"])
    rlib.ref_search_by_projection_sim3.restype = C.c_int
    n = rlib.ref_search_by_projection_sim3(_p(c(kps["x"])), _p(c(kps["y"])), _p(c(kps["octave"])), _p(s["desc"]), N, *trm.fb, _p(s["sf"]), _p(s["isig"]), _p(s["K4"]),
                                           _p(s["S"]), s["n_pts"], _p(s["Xw"]), _p(s["normal"]), _p(s["dmin"]), _p(s["dmax"]), _p(s["pdesc"]), _p(case["existing"]),
                                           int(th), _p(got), _p(valid), _p(u), _p(v), _p(lvl))
    return n, got, valid, u, v, lvl


def expected_reeval(table_words, skip, matched_after):
    """the points resolve has to evaluate again, from the outputs: a hit word on a feature that an EARLIER point of the call ended up claiming"""
    t = fs.unpack_table(table_words)
    n = 0
    for i in np.flatnonzero(t["status"] == 7):
        if skip is not None and skip[i]:
            continue
        j = int(matched_after[t["idx"][i]])
        n += 0 <= j < i
    return n


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the pair scene (M10)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def pair_case(frames):
    kps, desc = frames[0]
    N = len(kps)
    rng = np.random.default_rng(10)
    sf, _, _, isig = synth.scale_tables()
    K4e = np.array(synth.EUROC_K, np.float32)

    def rot(ax, a):
        ax = np.asarray(ax, float) / np.linalg.norm(ax)
        Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx

    R1, t1 = rot([0, 1, 0], 0.2), np.array([0.1, 0.0, 0.3])
    R2, t2 = rot([1, 0, 0], -0.4), np.array([-2.0, 1.0, 0.5])
    s12, R12, t12 = 1.15, rot([0.2, 1, 0.1], 0.03), np.array([0.05, -0.02, 0.1])
    sR21 = (1.0 / s12) * R12.T
    t21 = -sR21 @ t12
    z = rng.uniform(3, 9, N)
    Xc1 = np.stack([(kps["x"] - K4e[2]) / K4e[0] * z, (kps["y"] - K4e[3]) / K4e[1] * z, z], 1)
    Xc2 = Xc1 @ sR21.T + t21
    perm = rng.permutation(N)
    u2 = K4e[0] * Xc2[:, 0] / Xc2[:, 2] + K4e[2] + rng.normal(0, 1.0, N)
    v2 = K4e[1] * Xc2[:, 1] / Xc2[:, 2] + K4e[3] + rng.normal(0, 1.0, N)
    outside = (u2 < 1) | (u2 > 750) | (v2 < 1) | (v2 > 478)
    u2[outside] = rng.uniform(1, 750, outside.sum()); v2[outside] = rng.uniform(1, 478, outside.sum())
    F = lambda a: c(np.asarray(a, np.float32))
    kx2, ky2, oc2 = F(u2[perm]), F(v2[perm]), c(kps["octave"][perm])
    bits = np.unpackbits(desc, axis=1)
    desc2 = c(np.packbits(bits ^ (rng.random(bits.shape) < 0.06), axis=1)[perm])
    Xw1 = (Xc1 + rng.normal(0, 0.004, Xc1.shape) - t1) @ R1
    Xc2p = np.stack([(kx2 - K4e[2]) / K4e[0], (ky2 - K4e[3]) / K4e[1], np.ones(N)], 1) * Xc2[perm][:, 2:3]
    Xw2 = (Xc2p - t2) @ R2
    lvl1 = np.clip(kps["octave"] + rng.integers(0, 2, N), 0, 7); lvl2 = np.clip(oc2 + rng.integers(0, 2, N), 0, 7)
    d1 = np.linalg.norm(Xc2, axis=1); d2 = np.linalg.norm(Xc2p @ (s12 * R12).T + t12, axis=1)
    dmax1 = d1 * 1.2 ** (lvl1 - 0.5); dmax2 = d2 * 1.2 ** (lvl2 - 0.5)
    dmax1[:30] = d1[:30] * 0.3
    mdesc1 = c(np.packbits(bits ^ (rng.random(bits.shape) < 0.03), axis=1))
    mdesc2 = c(np.packbits(np.unpackbits(desc2, axis=1) ^ (rng.random(bits.shape) < 0.03), axis=1))
    has1 = (rng.random(N) < 0.8).astype(np.uint8); has2 = (rng.random(N) < 0.8).astype(np.uint8)
    inv = np.empty(N, np.int64); inv[perm] = np.arange(N)
    pre12 = -np.ones(N, np.int32)
    pre = rng.choice(np.flatnonzero(has2[inv] > 0), 60, replace=False)
    pre12[pre] = inv[pre]
    T1 = np.eye(4, dtype=np.float32); T1[:3, :3] = R1; T1[:3, 3] = t1
    T2 = np.eye(4, dtype=np.float32); T2[:3, :3] = R2; T2[:3, 3] = t2
    return dict(N=N, kps=kps, desc=desc, sf=sf, isig=isig, K4=K4e, kx2=kx2, ky2=ky2, oc2=oc2, desc2=desc2, T1=T1, T2=T2, has1=has1, has2=has2, Xw1=F(Xw1), Xw2=F(Xw2),
                dmin1=F(dmax1 / 1.2 ** 7), dmax1=F(dmax1), dmin2=F(dmax2 / 1.2 ** 7), dmax2=F(dmax2), mdesc1=mdesc1, mdesc2=mdesc2, s12=1.15, R12=F(R12), t12=F(t12),
                pre12=pre12, th=7.5)


def ref_pair(rlib, p):
    """the reference's own SearchBySim3: (n, matches12 on exit, (valid, u, v, level) of direction 1 -> 2, the same of 2 -> 1)"""
    N = p["N"]; kps = p["kps"]
    out12 = np.zeros(N, np.int32)
    d1 = trm._proj_out(N); d2 = trm._proj_out(N)
    rlib.ref_search_by_sim3.restype = C.c_int
    n = rlib.ref_search_by_sim3(_p(c(kps["x"])), _p(c(kps["y"])), _p(c(kps["octave"])), _p(p["desc"]), N, _p(p["T1"]), _p(p["has1"]), _p(p["Xw1"]), _p(p["dmin1"]),
                                _p(p["dmax1"]), _p(p["mdesc1"]), _p(p["kx2"]), _p(p["ky2"]), _p(p["oc2"]), _p(p["desc2"]), N, _p(p["T2"]), _p(p["has2"]), _p(p["Xw2"]),
                                _p(p["dmin2"]), _p(p["dmax2"]), _p(p["mdesc2"]), *trm.fb, _p(p["sf"]), _p(p["isig"]), _p(p["K4"]), C.c_float(p["s12"]), _p(p["R12"]),
                                _p(p["t12"]), C.c_float(p["th"]), _p(p["pre12"]), _p(out12), *[_p(a) for a in d1], *[_p(a) for a in d2])
    return n, out12, d1, d2


def pair_keyframes(p) -> fs.Scene:
    """keyframes 1 and 2 of the case with the caller's grids"""
    kps = p["kps"]
    return ss.keyframes_scene([(np.stack([kps["x"], kps["y"]], 1), kps["octave"], p["desc"]), (np.stack([p["kx2"], p["ky2"]], 1), p["oc2"], p["desc2"])], p["K4"],
                              trm.BOUNDS, p["sf"])


def pair_all_points(p, kfs: fs.Scene) -> ss.PairScene:
    """EVERY feature slot's point of both keyframes (the driver reports the gates of all of them): job 0 = keyframe 1's into keyframe 2, job 1 the other way"""
    N = p["N"]
    sR12, sR21, t21 = ss.derive(p["s12"], p["R12"], p["t12"])
    jobs = [(1, p["K4"], ss.pose12(p["T1"]), np.concatenate([sR21, t21]), 0, N), (0, p["K4"], ss.pose12(p["T2"]), np.concatenate([sR12, p["t12"].reshape(-1)]), N, N)]
    return ss.PairScene(kfs, p["th"], np.concatenate([p["Xw1"], p["Xw2"]]), np.concatenate([p["dmin1"], p["dmin2"]]), np.concatenate([p["dmax1"], p["dmax2"]]),
                        np.concatenate([p["mdesc1"], p["mdesc2"]]), jobs)


def pair_sides(p):
    return (ss.Side(p["has1"], p["Xw1"], p["dmin1"], p["dmax1"], p["mdesc1"], ss.pose12(p["T1"])),
            ss.Side(p["has2"], p["Xw2"], p["dmin2"], p["dmax2"], p["mdesc2"], ss.pose12(p["T2"])))


def same_gates_as_reference(res, j, n, has, ref_dir, tag):
    """job j's rows (n points, one per feature slot) against the driver's valid, u, v, level where the slot holds a point; every comparison exact"""
    valid, u, v, lvl = ref_dir
    a = int(res["off"][j])
    t = fs.unpack_table(res["table"][a:a + n]); uv = res["uv"][a:a + n]
    h = has > 0
    assert np.array_equal((t["status"] >= 4)[h], valid[h] > 0), tag
    m = h & (valid > 0)
    assert m.sum() > 0, tag
    assert np.array_equal(uv[m, 0].view(np.uint32), u[m].view(np.uint32)) and np.array_equal(uv[m, 1].view(np.uint32), v[m].view(np.uint32)), tag
    assert np.array_equal(t["level"][m], lvl[m]), tag


# ---------------------------------------------------------------------------------------------------------------------------------------------
# planted pairs of the SearchBySim3 gate
# ---------------------------------------------------------------------------------------------------------------------------------------------
class PairPlanted:
    """keyframes with hand-made features, groups of points with one job each; expect[(job, e)] = (status, idx or None, dist or None, level or None)"""

    def __init__(self, nlevels=8):
        self.sf = synth.scale_tables(nlevels)[0]
        self.kfs = []; self.pts = []; self.jobs = []; self.expect = {}

    def kf(self, feats=(), K4_=K4, bounds=trm.BOUNDS):
        xy = np.array([f[0] for f in feats], np.float32).reshape(-1, 2)
        self.kfs.append((xy, np.array([f[1] for f in feats], np.uint8), np.array([f[2] for f in feats], np.uint8).reshape(-1, 32), np.asarray(K4_, np.float32), bounds))
        return len(self.kfs) - 1

    def job(self, kf, pts, K4_=K4, src=IDENT12, T=IDENT12):
        """pts: [(pos, dmin, dmax, desc or None, expect)]"""
        j = len(self.jobs)
        self.jobs.append((kf, np.asarray(K4_, np.float32), np.asarray(src, np.float32), np.asarray(T, np.float32), len(self.pts), len(pts)))
        for e, (pos, dmin, dmax, desc, exp) in enumerate(pts):
            self.pts.append((np.asarray(pos, np.float32), f32(dmin), f32(dmax), np.zeros(32, np.uint8) if desc is None else np.asarray(desc, np.uint8)))
            self.expect[j, e] = exp
        return j

    def scene(self):
        off = [0]; xy = []; oc = []; de = []; co = []; ci = []; rec = []
        for kxy, koc, kde, k4, bounds in self.kfs:
            g = fs.build_grid(kxy, bounds)
            off.append(off[-1] + len(koc)); xy.append(kxy.reshape(-1)); oc.append(koc); de.append(kde.reshape(-1)); co.append(g[0]); ci.append(g[1])
            rec.append(fs.kf_record(k4, bounds))
        cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
        K = len(self.kfs); z = np.zeros(0, np.float32)
        kfs = fs.Scene(cat(rec, np.float32), off, cat(xy, np.float32), cat(oc, np.uint8), cat(de, np.uint8), cat(co, np.int32), cat(ci, np.int32),
                       np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), K), self.sf, fs.log_scale_factor(self.sf), 4.0, z, z, z, z, np.zeros(0, np.uint8))
        p = self.pts
        return ss.PairScene(kfs, 4.0, np.array([q[0] for q in p], np.float32), np.array([q[1] for q in p], np.float32), np.array([q[2] for q in p], np.float32),
                            np.array([q[3] for q in p], np.uint8), self.jobs)

    def check(self, res, tag=""):
        t = fs.unpack_table(res["table"])
        for (j, e), (st, idx, dist, lvl) in self.expect.items():
            w = int(res["off"][j]) + e
            got = (int(t["status"][w]), int(t["idx"][w]), int(t["dist"][w]), int(t["level"][w]))
            assert got[0] == st, (tag, j, e, got, st)
            for g, x in zip(got[1:], (idx, dist, lvl)):
                assert x is None or g == x, (tag, j, e, got, (st, idx, dist, lvl))


def pair_planted():
    rng = np.random.default_rng(6)
    q = rng.integers(0, 256, 32, dtype=np.uint8)
    pl = PairPlanted()
    k0 = pl.kf()                                                     # no features: a pair that passes the gates ends as status 4
    E = lambda st, idx=-1, dist=-1, lvl=None: (st, idx, dist, lvl)
    # depth: z == 0 is not behind the camera (invz = inf: the projection is NaN or inf, outside the image); z < 0 is.  z = -inf makes the first gemm's x and y
    # NaN (0 * inf), which the second gemm carries into its z: NaN < 0 is false, so that point is outside the image, not behind the camera
    pts = [((0, 0, 0), 1e-3, 1.0, None, E(1)), ((1, 0, 0), 1e-3, 1.0, None, E(1)), ((0, 0, -1), 1e-3, 1.0, None, E(0)), ((0, 0, -np.inf), 1e-3, 4.0, None, E(1)),
           ((np.nan, 0, 4), 1e-3, 4.0, None, E(1))]
    # both image bounds at depth 4 on the target's int bounds 0, 0, 752, 480: u = 16 X + 304, v = 16 Y + 224
    for pos, st in (((-19, 0, 4), 4), ((28, 0, 4), 1), ((0, -14, 4), 4), ((0, 16, 4), 1), ((np.nextafter(f32(-19), f32(-20)), 0, 4), 1), ((27.5, 0, 4), 4),
                    ((0, np.nextafter(f32(-14), f32(-15)), 4), 1), ((0, 15.5, 4), 4)):
        pts.append((pos, 1e-3, 64.0, None, E(st)))
    pl.job(k0, pts)
    # the range on the NORM OF THE CAMERA POINT: t_ba = (0, 0, 1) puts X = (0, 0, z - 1) at depth z, so the distance to the source camera's centre, z - 1, is outside
    # the range in every case and would be refused by a test on it
    lo = f32(0.8) * f32(5.0); hi = f32(1.2) * f32(5.0)
    T = IDENT12.copy(); T[11] = 1.0
    pts = []
    for z, st, dmin, dmax in ((lo, 4, 5.0, 50.0), (np.nextafter(lo, f32(0)), 2, 5.0, 50.0), (hi, 4, 0.1, 5.0), (np.nextafter(hi, f32(9)), 2, 0.1, 5.0)):
        zs = f32(f32(z) - f32(1))
        assert f32(zs + f32(1)) == f32(z)
        pts.append(((0, 0, zs), dmin, dmax, None, E(st)))
    pl.job(k0, pts, T=T)
    # the Hamming threshold TH_HIGH: one feature under the projection (304, 224), 100 and 101 bits away; and the level filter at levels 0, 3, 7
    p0 = (on_axis(4), 1e-3, 4.0, q); p3 = (on_axis(4), 1e-3, 4 * 1.2 ** 2.5, q); p7 = (on_axis(4), 1e-3, 4000.0, q)
    for nb, st in ((0, 7), (50, 7), (51, 7), (100, 7), (101, 6), (256, 6)):
        k = pl.kf([((304.0, 224.0), 0, _flip(q, nb))])
        pl.job(k, [p0 + (E(st, 0, nb, 0),), p3 + (E(5, -1, -1, 3),)])
    for o, st3, st0, st7 in ((0, 5, 7, 5), (1, 5, 5, 5), (2, 7, 5, 5), (3, 7, 5, 5), (4, 5, 5, 5), (6, 5, 5, 7), (7, 5, 5, 7)):
        k = pl.kf([((304.0, 224.0), o, _flip(q, 3))])
        hit = lambda st, lvl: E(st, 0 if st == 7 else -1, 3 if st == 7 else -1, lvl)
        pl.job(k, [p0 + (hit(st0, 0),), p3 + (hit(st3, 3),), p7 + (hit(st7, 7),)])
    # the job's K4, the target's bounds: the record of this keyframe says fx = fy = 64, cx = 304, cy = 224 and bounds 0, 0, 200, 200; the job projects with
    # fx = fy = 32, cx = cy = 100.  (1, 0, 4) lands on (108, 100), where the feature is (the record's K4 would put it on (320, 224), outside these bounds);
    # (16, 0, 4) lands on (228, 100): outside the target's 200 px, inside the 752 px of every other keyframe
    kb = pl.kf([((108.0, 100.0), 0, _flip(q, 5))], bounds=(0.0, 0.0, 200.0, 200.0))
    pl.job(kb, [((1, 0, 4), 1e-3, float(np.linalg.norm([1, 0, 4])), q, E(7, 0, 5, 0)), ((16, 0, 4), 1e-3, 64.0, q, E(1))], K4_=(32.0, 32.0, 100.0, 100.0))
    pl.job(kb, [((1, 0, 4), 1e-3, float(np.linalg.norm([1, 0, 4])), q, E(1))])      # the same point with the record's K4 in the job
    return pl


def angle_rejected_by_fuse():
    """a Planted scene (fuse_sim3_cases) with one on-axis point whose normal looks away: Fuse's viewing-angle gate refuses it (status 3)"""
    pl = Planted()
    k = pl.kf()
    pl.expect[k, pl.pt(on_axis(4), normal=(0, 0, -1), dmax=4)] = (3, -1, -1, None)
    return pl
