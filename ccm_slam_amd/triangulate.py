"""Triangulation of LocalMapping's new map points: the arithmetic between SearchForTriangulation and `new MapPoint` in
LocalMapping::CreateNewMapPoints (cslam/src/Mapping.cpp:353-448).

triangulate_pairs runs ccm_triangulate_pairs (one launch: every match of up to 20 neighbours, each its gate status and point);
triangulate_pairs_host runs the same lines compiled for the host (libccm_host.so).  NewMapPoints is the host mirror cslam::NewMapPointBatch:
the predicted matches of all neighbours in one launch at build time, points(j, pairs) answers the matches neighbour j has when its turn comes.

The generators below make two-view and multi-neighbour scenes: poses, points with pixel noise, per-match octaves, a share of gross mismatches,
points behind a camera, neighbours with a tiny baseline, and planted on-threshold cases.  They only produce numpy arrays.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional, Sequence

import numpy as np

from . import synth
from ._lib import CcmError, Context, _p, check, host, lib

STATUS = ("accepted", "parallax", "w == 0", "z1 <= 0", "z2 <= 0", "reprojection 1", "reprojection 2", "zero distance", "scale ratio")
CAM_FLOATS = 21

@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    h.ccmh_newpts_create.restype = C.c_void_p
    h.ccmh_newpts_create.argtypes = [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 4 + [C.c_float]
    h.ccmh_newpts_create_tri.restype = C.c_void_p
    h.ccmh_newpts_create_tri.argtypes = [C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 4 + [C.c_float]
    h.ccmh_newpts_points.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 3
    h.ccmh_newpts_stats.argtypes = [C.c_void_p, C.c_void_p]
    h.ccmh_newpts_destroy.argtypes = [C.c_void_p]
    h.ccmh_newpts_destroy.restype = None
    h.ccmh_triangulate_pairs_host.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 3
    return h


def _f32(a, shape=(-1,)):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))


def _i32(a, shape=(-1,)):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(shape))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# camera records and level tables
# ---------------------------------------------------------------------------------------------------------------------------------------------
def cam_record(Rcw, tcw, K=synth.EUROC_K) -> np.ndarray:
    """21 floats: Rcw (row-major), tcw, Ow = -Rcw' tcw (f32, as KeyFrame::SetPose stores it), fx fy cx cy, invfx = 1.0f / fx, invfy."""
    R = np.asarray(Rcw, np.float32).reshape(3, 3)
    t = np.asarray(tcw, np.float32).reshape(3)
    Ow = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(np.float32)
    fx, fy, cx, cy = (np.float32(v) for v in K)
    return np.concatenate([R.reshape(-1), t, Ow, [fx, fy, cx, cy, np.float32(1.0) / fx, np.float32(1.0) / fy]]).astype(np.float32)


def level_tables():
    """(mvLevelSigma2, mvScaleFactors) of the 8 x 1.2 pyramid."""
    sf, _, s2, _ = synth.scale_tables()
    return s2, sf


def ratio_factor(scale: float = synth.SCALE) -> np.float32:
    """1.5f * mfScaleFactor (Mapping.cpp:307)"""
    return np.float32(np.float32(1.5) * np.float32(scale))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the flat calls
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _flat_args(cam1, cam2, pair_off, xy, oct_, sigma2_1, sf_1, sigma2_2, sf_2):
    cam1 = _f32(cam1); cam2 = _f32(cam2); pair_off = _i32(pair_off); xy = _f32(xy); oct_ = _i32(oct_)
    t = [_f32(x) for x in (sigma2_1, sf_1, sigma2_2, sf_2)]
    S = pair_off.size - 1
    if cam1.size != CAM_FLOATS or cam2.size != CAM_FLOATS * S or len({x.size for x in t}) != 1:
        raise ValueError("camera records hold 21 floats each, one per group; the four level tables have one length")
    P = int(pair_off[-1]) if S >= 1 and np.all(np.diff(pair_off) >= 0) else 0
    if P and (xy.size != 4 * P or oct_.size != 2 * P):
        raise ValueError("xy holds 4 floats and oct 2 integers per match")
    return cam1, cam2, pair_off, xy, oct_, t, S, P


def triangulate_pairs(ctx: Context, cam1, cam2, pair_off, xy, oct_, sigma2_1, sf_1, sigma2_2, sf_2, ratio):
    """ccm_triangulate_pairs.  Returns (status[P] u8, x3d[P, 3] f32, n_accepted[S])."""
    cam1, cam2, pair_off, xy, oct_, t, S, P = _flat_args(cam1, cam2, pair_off, xy, oct_, sigma2_1, sf_1, sigma2_2, sf_2)
    status = np.zeros(max(P, 1), np.uint8); x3d = np.zeros((max(P, 1), 3), np.float32); nacc = np.zeros(max(S, 1), np.int32)
    check(lib().ccm_triangulate_pairs(ctx.handle, _p(cam1), int(S), _p(cam2), _p(pair_off), _p(xy), _p(oct_), int(t[0].size), _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]),
                                      C.c_float(ratio), _p(status), _p(x3d), _p(nacc)), ctx.handle)
    return status[:P], x3d[:P], nacc[:S]


def triangulate_pairs_host(cam1, cam2, pair_off, xy, oct_, sigma2_1, sf_1, sigma2_2, sf_2, ratio):
    """The same arguments through tri_pair compiled for the host, on the calling thread (ccmh_triangulate_pairs_host)."""
    cam1, cam2, pair_off, xy, oct_, t, S, P = _flat_args(cam1, cam2, pair_off, xy, oct_, sigma2_1, sf_1, sigma2_2, sf_2)
    status = np.zeros(max(P, 1), np.uint8); x3d = np.zeros((max(P, 1), 3), np.float32); nacc = np.zeros(max(S, 1), np.int32)
    rc = _host().ccmh_triangulate_pairs_host(_p(cam1), int(S), _p(cam2), _p(pair_off), _p(xy), _p(oct_), int(t[0].size), _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]),
                                             float(ratio), _p(status), _p(x3d), _p(nacc))
    if rc != 0:
        raise CcmError(f"ccmh_triangulate_pairs_host: bad arguments ({rc})")
    return status[:P], x3d[:P], nacc[:S]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cslam::NewMapPointBatch
# ---------------------------------------------------------------------------------------------------------------------------------------------
class NewMapPoints:
    """cslam::NewMapPointBatch.  keys = (x, y, octave) arrays of mvKeysUn; predicted[j] = (n, 2) feature index pairs of neighbour j as the flags of the
    build give them.  device=None asks for the host evaluator by name (no device is touched)."""

    def __init__(self, device: Optional[int], cam1, keys1, cam2, keys2: Sequence, predicted: Sequence, sigma2_1, sf_1, sigma2_2, sf_2, ratio):
        n_nb = len(keys2)
        k1 = (_f32(keys1[0]), _f32(keys1[1]), _i32(keys1[2]))
        k2 = [(_f32(k[0]), _f32(k[1]), _i32(k[2])) for k in keys2]
        pred = [_i32(p, (-1, 2)) for p in predicted]
        off = np.zeros(n_nb + 1, np.int32)
        off[1:] = np.cumsum([len(p) for p in pred])
        idx12 = _i32(np.concatenate(pred) if pred else np.zeros((0, 2)))
        N2 = _i32([k[0].size for k in k2])
        ptrs = lambda i: (C.c_void_p * max(n_nb, 1))(*[k[i].ctypes.data for k in k2])
        t = [_f32(x) for x in (sigma2_1, sf_1, sigma2_2, sf_2)]
        cam1 = _f32(cam1); cam2 = _f32(cam2)
        if cam1.size != CAM_FLOATS or cam2.size != CAM_FLOATS * n_nb:
            raise ValueError("camera records hold 21 floats each, one per neighbour")
        self._keep = (k1, k2, idx12)
        self._h = _host().ccmh_newpts_create(-1 if device is None else int(device), _p(cam1), int(k1[0].size), _p(k1[0]), _p(k1[1]), _p(k1[2]), n_nb, _p(cam2), _p(N2),
                                             ptrs(0), ptrs(1), ptrs(2), _p(off), _p(idx12), int(t[0].size), _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), float(ratio))
        if not self._h:
            raise CcmError("ccmh_newpts_create failed (bad arguments or no device)")

    @classmethod
    def from_tri_batch(cls, device: int, tri_batch_handle, oct1, cam1, cam2, F12, exy, sigma2_1, sf_1, sigma2_2, sf_2, ratio):
        """The prediction taken from a ccmh_tri_batch handle: every neighbour resolved with the flags of the batch's build."""
        self = cls.__new__(cls)
        t = [_f32(x) for x in (sigma2_1, sf_1, sigma2_2, sf_2)]
        a = [_i32(oct1), _f32(cam1), _f32(cam2), _f32(F12), _f32(exy)]
        self._keep = a
        self._h = _host().ccmh_newpts_create_tri(int(device), C.c_void_p(tri_batch_handle), *(_p(x) for x in a), int(t[0].size), _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]),
                                                 float(ratio))
        if not self._h:
            raise CcmError("ccmh_newpts_create_tri failed (bad arguments or no device)")
        return self

    def points(self, j: int, pairs):
        """(status[n], x3d[n, 3], number accepted) of the matches neighbour j has now."""
        p = _i32(pairs, (-1, 2))
        n = len(p)
        status = np.zeros(max(n, 1), np.uint8); x3d = np.zeros((max(n, 1), 3), np.float32)
        rc = _host().ccmh_newpts_points(self._h, int(j), n, _p(p), _p(status), _p(x3d))
        if rc < 0:
            raise CcmError(f"ccmh_newpts_points failed ({rc})")
        return status[:n], x3d[:n], rc

    def stats(self):
        """(predicted, hit, missed) matches"""
        out = np.zeros(3, np.int64)
        _host().ccmh_newpts_stats(self._h, _p(out))
        return tuple(int(x) for x in out)

    def close(self):
        if getattr(self, "_h", None):
            _host().ccmh_newpts_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _rot(w):
    """Rodrigues' formula in f64 for one rotation vector"""
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _pose(rng, centre, rot_sigma):
    """(Rcw, tcw) in f32 of a camera at `centre` looking roughly along +z."""
    R = _rot(rng.normal(0, rot_sigma, 3))
    t = -R @ np.asarray(centre, np.float64)
    return R.astype(np.float32), t.astype(np.float32)


def _project(R, t, X, K):
    Xc = X @ R.astype(np.float64).T + t.astype(np.float64)
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], 1), Xc[:, 2]


def make_pair_scene(seed: int = 0, S: int = 4, n_pairs=200, noise_px: float = 0.6, mismatch: float = 0.08, behind: float = 0.04, tiny_baseline: float = 0.15,
                    wild_octave: float = 0.05, empty: Sequence[int] = (), K=synth.EUROC_K):
    """One new keyframe and S neighbours with their matches, laid out for ccm_triangulate_pairs.  n_pairs: an int or one count per group (groups listed
    in `empty` get none).  mismatch: share of matches whose second keypoint is a random pixel; behind: share whose point lies behind both cameras;
    tiny_baseline: share of neighbours a few millimetres away (parallax gate); wild_octave: share of matches with unrelated octaves (scale gate).
    Returns a dict: cam1, cam2 (S, 21), pair_off, xy (P, 4), oct (P, 2), X (P, 3) planted points (NaN for mismatches), sigma2, sf, ratio."""
    rng = np.random.default_rng(seed)
    counts = [int(n_pairs)] * S if np.isscalar(n_pairs) else [int(n) for n in n_pairs]
    for e in empty:
        counts[e] = 0
    s2, sf = level_tables()
    R1, t1 = _pose(rng, rng.normal(0, 0.05, 3), 0.03)
    cam1 = cam_record(R1, t1, K)
    cam2, xy, octs, Xs = [], [], [], []
    for s in range(S):
        tiny = rng.random() < tiny_baseline
        base = rng.normal(0, 1, 3) * [1, 0.4, 0.3]
        base *= (rng.uniform(0.001, 0.004) if tiny else rng.uniform(0.15, 0.6)) / np.linalg.norm(base)
        R2, t2 = _pose(rng, base, 0.04)
        cam2.append(cam_record(R2, t2, K))
        n = counts[s]
        if n == 0:
            continue
        depth = rng.uniform(1.5, 9.0, n)
        px = np.stack([rng.uniform(40, synth.IMG_W - 40, n), rng.uniform(40, synth.IMG_H - 40, n)], 1)
        Xc = np.stack([(px[:, 0] - K[2]) / K[0] * depth, (px[:, 1] - K[3]) / K[1] * depth, depth], 1)
        is_behind = rng.random(n) < behind
        Xc[is_behind] *= -1                                           # the same pixels, the point behind the camera
        X = (Xc - t1.astype(np.float64)) @ R1.astype(np.float64)      # Rwc (Xc - tcw)
        o1 = rng.integers(0, synth.N_LEVELS, n)
        o2 = np.clip(o1 + rng.integers(-1, 2, n), 0, synth.N_LEVELS - 1)
        wild = rng.random(n) < wild_octave
        o2[wild] = rng.integers(0, synth.N_LEVELS, int(wild.sum()))
        p1, _ = _project(R1, t1, X, K)
        p2, _ = _project(R2, t2, X, K)
        p1 += rng.normal(0, noise_px, (n, 2)) * sf[o1][:, None]
        p2 += rng.normal(0, noise_px, (n, 2)) * sf[o2][:, None]
        bad = rng.random(n) < mismatch
        p2[bad] = np.stack([rng.uniform(0, synth.IMG_W, int(bad.sum())), rng.uniform(0, synth.IMG_H, int(bad.sum()))], 1)
        X[bad] = np.nan
        xy.append(np.concatenate([p1, p2], 1)); octs.append(np.stack([o1, o2], 1)); Xs.append(X)
    pair_off = np.zeros(S + 1, np.int32)
    pair_off[1:] = np.cumsum(counts)
    cat = lambda a, w, dt: np.ascontiguousarray(np.concatenate(a) if a else np.zeros((0, w)), dt)
    return dict(cam1=cam1, cam2=np.ascontiguousarray(np.stack(cam2), np.float32), pair_off=pair_off, xy=cat(xy, 4, np.float32), oct=cat(octs, 2, np.int32),
                X=cat(Xs, 3, np.float64), sigma2=s2, sf=sf, ratio=ratio_factor())


def flat(sc: dict):
    """The positional arguments of triangulate_pairs / triangulate_pairs_host after the context."""
    return (sc["cam1"], sc["cam2"], sc["pair_off"], sc["xy"], sc["oct"], sc.get("sigma2_1", sc["sigma2"]), sc.get("sf_1", sc["sf"]), sc["sigma2"], sc["sf"], sc["ratio"])


# ---- planted cases --------------------------------------------------------------------------------------------------------------------------
def _cos_parallax(cam1, cam2, xy):
    """cosParallaxRays of Mapping.cpp:363-368 for an (n, 4) f32 array of matches (f32 rays, f64 quotient, f32 result), vectorised."""
    f = np.float32
    out = []
    for cam, x, y in ((cam1, xy[:, 0], xy[:, 1]), (cam2, xy[:, 2], xy[:, 3])):
        R = cam[:9].reshape(3, 3)
        a = ((x - cam[17]) * cam[19]).astype(f); b = ((y - cam[18]) * cam[20]).astype(f)
        out.append(np.stack([((R[0, r] * a).astype(f) + (R[1, r] * b).astype(f)).astype(f) + R[2, r] for r in range(3)], 1).astype(f).astype(np.float64))
    r1, r2 = out
    dot = r1[:, 0] * r2[:, 0]; n1 = r1[:, 0] * r1[:, 0]; n2 = r2[:, 0] * r2[:, 0]
    for k in (1, 2):
        dot = dot + r1[:, k] * r2[:, k]; n1 = n1 + r1[:, k] * r1[:, k]; n2 = n2 + r2[:, k] * r2[:, k]
    return (dot / (np.sqrt(n1) * np.sqrt(n2))).astype(f)


def plant_parallax_threshold(K=synth.EUROC_K, target=np.float32(0.9998)):
    """Two cameras 0.2 apart with identity rotation, keypoint 1 on the principal point, and keypoint 2's x scanned float by float until cosParallaxRays
    lands exactly on `target`: three matches with cos = the float below it, it, and the float above it.  Returns (cam1, cam2, xy (3, 4), cos (3,))."""
    cam1 = cam_record(np.eye(3), np.zeros(3), K)
    cam2 = cam_record(np.eye(3), [-0.2, 0, 0], K)
    a = np.sqrt(1.0 / float(target) ** 2 - 1.0)
    x0 = np.float32(cam2[17] + a * K[0])
    xs = [x0]
    lo = hi = x0
    for _ in range(4000):
        lo = np.nextafter(lo, np.float32(-np.inf)); hi = np.nextafter(hi, np.float32(np.inf))
        xs += [lo, hi]
    xs = np.sort(np.array(xs, np.float32))
    xy = np.zeros((xs.size, 4), np.float32)
    xy[:, 0] = cam1[17]; xy[:, 1] = cam1[18]; xy[:, 2] = xs; xy[:, 3] = cam2[18]
    cos = _cos_parallax(cam1, cam2, xy)
    want = [np.nextafter(target, np.float32(0)), target, np.nextafter(target, np.float32(2))]
    pick = []
    for w in want:
        hit = np.nonzero(cos == w)[0]
        if hit.size == 0:
            raise RuntimeError(f"no keypoint gives cos = {w!r}")
        pick.append(int(hit[0]))
    return cam1, cam2, xy[pick], cos[pick]


def plant_depth_zero(K=synth.EUROC_K):
    """Two cameras at the origin that differ by a rotation only: A's last column is zero, the SVD's last row is e4, x3D = 0 = both centres, z1 = 0 exactly.
    Returns (cam1, cam2, xy (1, 4))."""
    cam1 = cam_record(np.eye(3), np.zeros(3), K)
    cam2 = cam_record(_rot([0.0, 0.25, 0.0]), np.zeros(3), K)
    xy = np.array([[K[2] + 30, K[3] - 12, K[2] - 50, K[3] + 20]], np.float32)
    return cam1, cam2, xy


def plant_w_zero(K=synth.EUROC_K):
    """A record that makes vt.row(3)(3) exactly 0 although the rays are not parallel — which no rigid pose can: keypoint 1 on the principal point of an identity
    camera and a second `rotation` whose third column is (a2, b2, 1), so that A's third column cancels exactly and e3 is the null vector.  It exercises the
    reference's `x3D(3) == 0` line.  Returns (cam1, cam2, xy (1, 4))."""
    cam1 = cam_record(np.eye(3), np.zeros(3), K)
    cam2 = cam_record(np.eye(3), [-0.3, 0.1, 0.05], K)
    xy = np.array([[cam1[17], cam1[18], K[2] + 200, K[3] + 60]], np.float32)
    a2 = np.float32((xy[0, 2] - cam2[17]) * cam2[19]); b2 = np.float32((xy[0, 3] - cam2[18]) * cam2[20])
    cam2[2] = a2; cam2[5] = b2; cam2[8] = 1.0
    return cam1, cam2, xy


def sigma2_bracket(e2: np.float32):
    """Level tables that put 5.991 * sigma2 on the float e2 (a squared reprojection error) and one ulp of sigma2 to either side: octave 0 -> the
    threshold lies below e2 (gate fails), octave 1 -> the nearest sigma2, octave 2 -> above e2 (gate passes); the other octaves hold 1e6."""
    c = np.float32(float(e2) / 5.991)
    t = np.full(synth.N_LEVELS, 1e6, np.float32)
    t[0] = np.nextafter(c, np.float32(0)); t[1] = c; t[2] = np.nextafter(c, np.float32(np.inf))
    return t


# ---- keyframes with features, for the batch ---------------------------------------------------------------------------------------------------
def make_keyframe_scene(seed: int = 0, S: int = 6, n_feat: int = 300, shared: float = 0.6, rival: float = 0.5, disjoint: bool = False, noise_px: float = 0.5,
                        K=synth.EUROC_K):
    """A new keyframe with n_feat features and S neighbours that observe parts of the same points.  cands[j] = the candidate matches of neighbour j as
    (idx1, idx2) rows in matching order: the true match of every shared feature, and for a share `rival` of them a second feature of keyframe 1 that
    competes for the same idx2 (it gets it once the first has a map point); truth[j] = the true matches alone.  disjoint: every feature of keyframe 1 is seen by one neighbour only and
    has no rival.  Returns a dict: cam1, keys1 (x, y, oct), cam2 (S, 21), keys2 [(x, y, oct)], cands [(n, 2)], sigma2, sf, ratio."""
    rng = np.random.default_rng(seed)
    s2, sf = level_tables()
    R1, t1 = _pose(rng, np.zeros(3), 0.02)
    depth = rng.uniform(2.0, 8.0, n_feat)
    px = np.stack([rng.uniform(60, synth.IMG_W - 60, n_feat), rng.uniform(60, synth.IMG_H - 60, n_feat)], 1)
    Xc = np.stack([(px[:, 0] - K[2]) / K[0] * depth, (px[:, 1] - K[3]) / K[1] * depth, depth], 1)
    X = (Xc - t1.astype(np.float64)) @ R1.astype(np.float64)
    o1 = rng.integers(0, synth.N_LEVELS, n_feat)
    p1 = px + rng.normal(0, noise_px, (n_feat, 2)) * sf[o1][:, None]
    cam2, keys2, cands, truth = [], [], [], []
    owner = rng.integers(0, S, n_feat)
    for j in range(S):
        base = rng.normal(0, 1, 3) * [1, 0.4, 0.2]
        base *= rng.uniform(0.2, 0.6) / np.linalg.norm(base)
        R2, t2 = _pose(rng, base, 0.03)
        cam2.append(cam_record(R2, t2, K))
        seen = np.nonzero(owner == j)[0] if disjoint else np.nonzero(rng.random(n_feat) < shared)[0]
        o2 = np.clip(o1[seen] + rng.integers(-1, 2, seen.size), 0, synth.N_LEVELS - 1)
        p2, _ = _project(R2, t2, X[seen], K)
        p2 += rng.normal(0, noise_px, (seen.size, 2)) * sf[o2][:, None]
        perm = rng.permutation(seen.size)                            # keyframe 2 numbers its features in its own order
        keys2.append((p2[perm, 0].astype(np.float32), p2[perm, 1].astype(np.float32), o2[perm].astype(np.int32)))
        inv = np.argsort(perm)
        rows = [(int(i1), int(inv[k])) for k, i1 in enumerate(seen)]
        truth.append(np.array(rows, np.int32).reshape(-1, 2))
        if not disjoint:
            for k, i1 in enumerate(seen):
                if rng.random() < rival:
                    rows.append((int(rng.integers(0, n_feat)), int(inv[k])))
        cands.append(np.array(sorted(set(rows)), np.int32).reshape(-1, 2))
    return dict(cam1=cam_record(R1, t1, K), keys1=(p1[:, 0].astype(np.float32), p1[:, 1].astype(np.float32), o1.astype(np.int32)),
                cam2=np.ascontiguousarray(np.stack(cam2), np.float32), keys2=keys2, cands=cands, truth=truth, X=X, sigma2=s2, sf=sf, ratio=ratio_factor())


def fundamental(cam1, cam2):
    """(F12 row-major 3x3 f32, epipole (ex, ey) of keyframe 1's centre in image 2) as LocalMapping::ComputeF12 (Mapping.cpp:769-790) and
    ORBmatcher.cpp:708-714 define them, computed in f64 from two camera records."""
    c1, c2 = np.asarray(cam1, np.float64), np.asarray(cam2, np.float64)
    R1, t1, R2, t2 = c1[:9].reshape(3, 3), c1[9:12], c2[:9].reshape(3, 3), c2[9:12]
    Km = lambda c: np.array([[c[15], 0, c[17]], [0, c[16], c[18]], [0, 0, 1]])
    R12 = R1 @ R2.T
    t12 = -R12 @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = np.linalg.inv(Km(c1)).T @ tx @ R12 @ np.linalg.inv(Km(c2))
    C2 = R2 @ c1[12:15] + t2
    return F12.astype(np.float32).reshape(-1), (float(c2[15] * C2[0] / C2[2] + c2[17]), float(c2[16] * C2[1] / C2[2] + c2[18]))


def resolve_candidates(cands: np.ndarray, has1: np.ndarray) -> np.ndarray:
    """A stand-in for SearchForTriangulation's sequential rules on a candidate list: features of keyframe 1 in ascending order, those with a map point
    skipped, each taking its first candidate idx2 that no earlier feature has claimed.  Returns (n, 2) pairs in ascending idx1."""
    claimed = set()
    out = []
    last = -1
    for i1, i2 in cands:                                             # sorted by (idx1, idx2)
        if has1[i1] or i1 == last or int(i2) in claimed:
            continue
        claimed.add(int(i2)); out.append((int(i1), int(i2))); last = i1
    return np.array(out, np.int32).reshape(-1, 2)


def pairs_to_flat(sc: dict, j: int, pairs: np.ndarray):
    """xy (n, 4) and oct (n, 2) of the matches `pairs` of neighbour j of a keyframe scene."""
    k1, k2 = sc["keys1"], sc["keys2"][j]
    i1, i2 = pairs[:, 0], pairs[:, 1]
    return (np.stack([k1[0][i1], k1[1][i1], k2[0][i2], k2[1][i2]], 1).astype(np.float32), np.stack([k1[2][i1], k2[2][i2]], 1).astype(np.int32))
