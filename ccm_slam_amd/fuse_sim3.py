"""SearchAndFuse of a loop closure or a map merge (cslam/src/LoopFinder.cpp:709-734, MapMerger.cpp:574-598): ORBmatcher::Fuse(pKF, Scw, vpLoopMapPoints, th,
vpReplacePoints) (ORBmatcher.cpp:995-1122) for every keyframe of CorrectedSim3 against the same points.

fuse_sim3_eval runs ccm_fuse_sim3_eval (every (keyframe, point) pair in one launch), fuse_sim3_eval_host the same lines compiled for the host (libccm_host.so);
unpack_table splits the packed answers.  SearchAndFuseBatch is the host mirror cslam::SearchAndFuseBatch, whose resolve(k, ...) answers the k-th Fuse call.
build_grid makes a keyframe's mGrid as a CSR by the reference's AssignFeaturesToGrid rule.

make_scene / profile_scene generate keyframes and points as numpy arrays; nothing in them touches the device.
"""
from __future__ import annotations

import ctypes as C
import ctypes.util
import functools
from typing import Optional

import numpy as np

from . import synth
from ._lib import CcmError, Context, _p, check, host, lib

STATUS = ("behind the camera", "outside the image", "distance range", "viewing angle", "window empty", "no candidate at the level", "best distance > TH_LOW", "hit")
GRID_COLS, GRID_ROWS = 75, 48
CELLS = GRID_COLS * GRID_ROWS
NO_IDX, NO_DIST = 0xFFFF, 511


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    V = C.c_void_p
    ev = [C.c_int] + [V] * 8 + [C.c_int, V, C.c_float, C.c_float, C.c_int] + [V] * 5
    h.ccmh_fuse_sim3_create.restype = V
    h.ccmh_fuse_sim3_create.argtypes = [C.c_int] + ev
    h.ccmh_fuse_sim3_table.argtypes = [V] * 4
    h.ccmh_fuse_sim3_resolve.argtypes = [V, C.c_int, V, V, C.c_int, V, V]
    h.ccmh_fuse_sim3_n_reeval.argtypes = [V]
    h.ccmh_fuse_sim3_n_reeval.restype = C.c_longlong
    h.ccmh_fuse_sim3_destroy.argtypes = [V]
    h.ccmh_fuse_sim3_destroy.restype = None
    h.ccmh_fuse_sim3_eval_host.argtypes = ev + [V] * 5
    h.ccmh_fuse_sim3_decompose.argtypes = [V, V]
    h.ccmh_fuse_sim3_decompose.restype = None
    return h


@functools.lru_cache(maxsize=None)
def _dev():
    l = lib()
    V = C.c_void_p
    l.ccm_fuse_sim3_eval.argtypes = [V, C.c_int] + [V] * 8 + [C.c_int, V, C.c_float, C.c_float, C.c_int] + [V] * 9
    return l


def log_scale_factor(scale_factors) -> float:
    """mfLogScaleFactor = log(mfScaleFactor) as the reference computes it: the C library's logf of the f32 ratio of the first two levels"""
    sf = np.asarray(scale_factors, np.float32)
    ratio = np.float32(sf[1] / sf[0]) if sf.size > 1 else np.float32(synth.SCALE)
    m = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.logf.restype = C.c_float
    m.logf.argtypes = [C.c_float]
    return float(m.logf(C.c_float(ratio)))


def kf_record(K4, bounds) -> np.ndarray:
    """The 10 floats of one keyframe: fx fy cx cy, the int-truncated bounds (KeyFrame.cpp:54-57), the grid inverses of the Frame's float bounds (Frame.cpp:74-75).
    bounds = mnMinX mnMinY mnMaxX mnMaxY of the Frame."""
    b = np.asarray(bounds, np.float32)
    w_inv = np.float32(GRID_COLS) / np.float32(b[2] - b[0])
    h_inv = np.float32(GRID_ROWS) / np.float32(b[3] - b[1])
    return np.array(list(np.asarray(K4, np.float32)) + [np.float32(int(v)) for v in b] + [w_inv, h_inv], np.float32)


def build_grid(xy, bounds):
    """A keyframe's mGrid as (cell_off[3601], cell_idx[n]) from its undistorted keypoints and the Frame's float bounds: Frame::AssignFeaturesToGrid (Frame.cpp:103-118)
    with Frame::PosInGrid (:254-265, csrc/frame_math.h frame_cell_of): f32 arithmetic, round half away from zero, cells x-major, insertion order inside a cell.
    A keypoint outside the grid is in no cell; ccm_fuse_sim3_eval wants every feature in one, so such a keyframe is refused here: drop the keypoint first (the reference
    can never return it from GetFeaturesInArea)."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    b = np.asarray(bounds, np.float32)
    w_inv = np.float32(GRID_COLS) / np.float32(b[2] - b[0])
    h_inv = np.float32(GRID_ROWS) / np.float32(b[3] - b[1])
    tx = ((xy[:, 0] - b[0]).astype(np.float32) * w_inv).astype(np.float32).astype(np.float64)
    ty = ((xy[:, 1] - b[1]).astype(np.float32) * h_inv).astype(np.float32).astype(np.float64)
    rnd = lambda t: np.where(t >= 0, np.floor(t + 0.5), np.ceil(t - 0.5)).astype(np.int64)
    px, py = rnd(tx), rnd(ty)
    if ((px < 0) | (px >= GRID_COLS) | (py < 0) | (py >= GRID_ROWS)).any():
        raise ValueError("build_grid: a keypoint lies outside the grid")
    cell = px * GRID_ROWS + py
    order = np.argsort(cell, kind="stable")
    off = np.zeros(CELLS + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(cell, minlength=CELLS))
    return off, order.astype(np.int32)


def unpack_table(table) -> dict:
    """The packed answers as arrays of the table's shape: idx (-1 none), dist (-1 none), level, status"""
    t = np.asarray(table, np.uint32)
    idx = (t & 0xFFFF).astype(np.int32); dist = ((t >> 16) & 0x1FF).astype(np.int32)
    idx[idx == NO_IDX] = -1; dist[dist == NO_DIST] = -1
    return dict(idx=idx, dist=dist, level=((t >> 25) & 0xF).astype(np.int32), status=(t >> 29).astype(np.int32))


def _c(a, dt, n=None):
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a, dt).reshape(-1))
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} elements, got {a.size}")
    return a


class Scene:
    """The flat arguments of ccm_fuse_sim3_eval, checked for their lengths only (the values are the library's to check)"""

    def __init__(self, rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx, Scw, scale_factors, log_sf, th, pos, normal, min_dist, max_dist, pt_desc):
        self.feat_off = _c(feat_off, np.int32)
        self.K = K = max(self.feat_off.size - 1, 0) if rec is not None and np.size(rec) else 0
        F = int(self.feat_off[K]) if K and 0 <= int(self.feat_off[K]) < (1 << 31) else 0
        self.rec = _c(rec, np.float32, 10 * K)
        self.feat_xy = _c(feat_xy, np.float32); self.feat_octave = _c(feat_octave, np.uint8); self.feat_desc = _c(feat_desc, np.uint8)
        self.cell_off = _c(cell_off, np.int32, (CELLS + 1) * K); self.cell_idx = _c(cell_idx, np.int32)
        if self.feat_xy.size < 2 * F or self.feat_octave.size < F or self.feat_desc.size < 32 * F or self.cell_idx.size < F:
            raise ValueError("feature arrays shorter than feat_off says")
        self.Scw = _c(Scw, np.float32, 12 * K)
        self.scale_factors = _c(scale_factors, np.float32); self.nlevels = int(self.scale_factors.size)
        self.log_sf = float(log_sf); self.th = float(th)
        self.pos = _c(pos, np.float32); self.P = P = self.pos.size // 3
        self.normal = _c(normal, np.float32, 3 * P); self.min_dist = _c(min_dist, np.float32, P); self.max_dist = _c(max_dist, np.float32, P)
        self.pt_desc = _c(pt_desc, np.uint8, 32 * P)

    def args(self):
        return [self.K, _p(self.rec), _p(self.feat_off), _p(self.feat_xy), _p(self.feat_octave), _p(self.feat_desc), _p(self.cell_off), _p(self.cell_idx), _p(self.Scw),
                self.nlevels, _p(self.scale_factors), C.c_float(self.log_sf), C.c_float(self.th), self.P, _p(self.pos), _p(self.normal), _p(self.min_dist),
                _p(self.max_dist), _p(self.pt_desc)]

    def subset(self, kfs, n_pts: Optional[int] = None) -> "Scene":
        """the keyframes `kfs` (in that order) and the first n_pts points"""
        P = self.P if n_pts is None else int(n_pts)
        off = [0]; xy = []; oc = []; de = []; ci = []
        for k in kfs:
            a, b = int(self.feat_off[k]), int(self.feat_off[k + 1])
            xy.append(self.feat_xy[2 * a:2 * b]); oc.append(self.feat_octave[a:b]); de.append(self.feat_desc[32 * a:32 * b]); ci.append(self.cell_idx[a:b])
            off.append(off[-1] + b - a)
        cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dt)
        kfs = list(kfs)
        return Scene(self.rec.reshape(-1, 10)[kfs], off, cat(xy, np.float32), cat(oc, np.uint8), cat(de, np.uint8), self.cell_off.reshape(-1, CELLS + 1)[kfs],
                     cat(ci, np.int32), self.Scw.reshape(-1, 12)[kfs], self.scale_factors, self.log_sf, self.th, self.pos[:3 * P], self.normal[:3 * P], self.min_dist[:P],
                     self.max_dist[:P], self.pt_desc[:32 * P])


def _outputs(s: Scene, want_uv: bool):
    n = s.K * s.P
    return (np.zeros(n, np.uint32), np.zeros(s.K, np.int32), np.zeros(s.K, np.int32), np.zeros(2 * n, np.float32) if want_uv else None)


def _result(s: Scene, table, n_valid, n_hit, uv, n_cand=None):
    out = dict(table=table.reshape(s.K, s.P), n_valid=n_valid, n_hit=n_hit)
    if uv is not None:
        out["uv"] = uv.reshape(s.K, s.P, 2)
    if n_cand is not None:
        out["n_cand"] = n_cand.reshape(s.K, s.P)
    return out


def fuse_sim3_eval(ctx: Context, s: Scene, want_uv: bool = False) -> dict:
    """ccm_fuse_sim3_eval: table (K, P) packed, n_valid[K], n_hit[K] and, when asked for, uv (K, P, 2)"""
    table, nv, nh, uv = _outputs(s, want_uv)
    check(_dev().ccm_fuse_sim3_eval(ctx.handle, *s.args(), _p(table), _p(nv), _p(nh), _p(uv)), ctx.handle)
    return _result(s, table, nv, nh, uv)


def fuse_sim3_eval_host(s: Scene, want_uv: bool = False, want_cand: bool = False) -> dict:
    """The same through csrc/fuse_math.h on the calling thread; n_cand (K, P) = the size of vIndices per pair when asked for"""
    table, nv, nh, uv = _outputs(s, want_uv)
    nc = np.zeros(s.K * s.P, np.int32) if want_cand else None
    if _host().ccmh_fuse_sim3_eval_host(*s.args(), _p(table), _p(nv), _p(nh), _p(uv), _p(nc)) != 0:
        raise CcmError("ccmh_fuse_sim3_eval_host: bad arguments")
    return _result(s, table, nv, nh, uv, nc)


def decompose_scw(Scw12) -> np.ndarray:
    """ORBmatcher.cpp:1004-1008: Rcw (9), tcw (3), Ow (3) of rows 0..2 of Scw"""
    S = _c(Scw12, np.float32, 12); out = np.zeros(15, np.float32)
    _host().ccmh_fuse_sim3_decompose(_p(S), _p(out))
    return out


class SearchAndFuseBatch:
    """cslam::SearchAndFuseBatch: ONE evaluation of every pair at construction (ctx = None: the host evaluator), then resolve(k, ...) per Fuse call"""

    def __init__(self, ctx: Optional[Context], s: Scene, device: int = 0):
        self.scene = s
        self._h = _host().ccmh_fuse_sim3_create(-1 if ctx is None else int(getattr(ctx, "device", device)), *s.args())
        if not self._h:
            raise CcmError("ccmh_fuse_sim3_create failed (bad arguments or a device error)")

    def table(self) -> dict:
        s = self.scene
        table, nv, nh, _ = _outputs(s, False)
        _host().ccmh_fuse_sim3_table(self._h, _p(table), _p(nv), _p(nh))
        return _result(s, table, nv, nh, None)

    def resolve(self, k: int, skip_now=None, desc_now=None):
        """(nFused, bestIdx[P] (-1: not fused), bestDist[P]) of the k-th Fuse call"""
        P = self.scene.P
        skip = _c(skip_now, np.uint8, P) if skip_now is not None else None
        desc = _c(desc_now, np.uint8, 32 * P) if desc_now is not None else None
        bi = np.zeros(P, np.int32); bd = np.zeros(P, np.int32)
        n = _host().ccmh_fuse_sim3_resolve(self._h, int(k), _p(skip), _p(desc), P, _p(bi), _p(bd))
        if n < 0:
            raise CcmError(f"ccmh_fuse_sim3_resolve: {n}")
        return n, bi, bd

    def n_reeval(self) -> int:
        return int(_host().ccmh_fuse_sim3_n_reeval(self._h))

    def close(self):
        if self._h:
            _host().ccmh_fuse_sim3_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------------------------
BOUNDS = (0.0, 0.0, float(synth.IMG_W), float(synth.IMG_H))


def _rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float64)


def perturbed_scw(rng, scale: float, d_rad: float, d_m: float, ang: float = 0.3, t=(0.4, -0.2, 0.7)) -> np.ndarray:
    """Rows 0..2 of a Sim3 [s R | s t] around the pose of the scenes below, perturbed by d_rad about a random axis and d_m in translation"""
    R = synth.rodrigues((d_rad * rng.normal(size=3) / np.sqrt(3.0))[None])[0] @ _rot_y(ang)
    tt = np.asarray(t, np.float64) + d_m * rng.normal(size=3) / np.sqrt(3.0)
    S = np.zeros((3, 4), np.float64); S[:, :3] = scale * R; S[:, 3] = scale * tt
    return S.astype(np.float32).reshape(-1)


def assemble(frames, which, Scw, K4, scale_factors, th, pos, normal, min_dist, max_dist, pt_desc, bounds=BOUNDS) -> Scene:
    """A Scene from per-frame features: frames = [(xy (n, 2), octave, desc (n, 32))], which[k] = the frame keyframe k shows"""
    grids = [build_grid(f[0], bounds) for f in frames]
    rec = np.tile(kf_record(K4, bounds), (len(which), 1))
    off = [0]; xy = []; oc = []; de = []; co = []; ci = []
    for w in which:
        f = frames[w]
        n = len(f[1])
        off.append(off[-1] + n)
        xy.append(np.asarray(f[0], np.float32).reshape(-1)); oc.append(np.asarray(f[1], np.uint8)); de.append(np.asarray(f[2], np.uint8).reshape(-1))
        co.append(grids[w][0]); ci.append(grids[w][1])
    cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dt)
    return Scene(rec, off, cat(xy, np.float32), cat(oc, np.uint8), cat(de, np.uint8), cat(co, np.int32), cat(ci, np.int32), Scw, scale_factors, log_scale_factor(scale_factors),
                 th, pos, normal, min_dist, max_dist, pt_desc)


def make_scene(n_kf: int, n_pts: int, n_feat: int = 1000, seed: int = 0, th: float = 4.0, far_every: int = 4) -> Scene:
    """Two synthetic feature sets (n_feat keypoints each, octaves 0..7, random descriptors; the second is the first a few pixels on) seen alternately by n_kf
    keyframes around one pose; n_pts points back-projected from the first set with noisy copies of its descriptors.  Every far_every-th keyframe is "far" (0.08 rad, 0.25 m off), the others "near" (0.004 rad, 0.01 m); the Sim3
    scales cycle through 1.0, 1.7, 0.8, 1.2."""
    rng = np.random.default_rng(seed)
    sf = synth.scale_tables()[0]
    K4 = np.array(synth.EUROC_K, np.float32)
    xy = np.stack([rng.uniform(24, synth.IMG_W - 24, n_feat), rng.uniform(24, synth.IMG_H - 24, n_feat)], 1).astype(np.float32)
    octv = np.minimum(rng.geometric(0.35, n_feat) - 1, 7).astype(np.uint8)
    desc = rng.integers(0, 256, (n_feat, 32), dtype=np.uint8)
    # the second set: the same scene a moment later (shifted by a few pixels, shuffled, noisy copies of the descriptors)
    perm = rng.permutation(n_feat)
    xy2 = (xy[perm] + np.array([2.5, -1.5]) + rng.normal(0, 0.7, (n_feat, 2))).astype(np.float32)
    desc2 = np.packbits(np.unpackbits(desc[perm], axis=1) ^ (rng.random((n_feat, 256)) < 0.05), axis=1)
    frames = [(xy, octv, desc), (xy2, octv[perm], desc2)]
    R = _rot_y(0.3); t = np.array([0.4, -0.2, 0.7])
    src = rng.integers(0, n_feat, n_pts)
    z = rng.uniform(3, 9, n_pts)
    uu = frames[0][0][src, 0] + rng.normal(0, 1.5, n_pts); vv = frames[0][0][src, 1] + rng.normal(0, 1.5, n_pts)
    Xc = np.stack([(uu - K4[2]) / K4[0] * z, (vv - K4[3]) / K4[1] * z, z], 1)
    Xw = (Xc - t) @ R
    PO = Xw + R.T @ t
    dist = np.linalg.norm(PO, axis=1)
    normal = PO / dist[:, None]
    lvl = np.clip(frames[0][1][src].astype(int) + rng.integers(0, 2, n_pts), 0, 7)
    dmax = dist * 1.2 ** (lvl - 0.5)
    dmin = dmax / 1.2 ** 7
    bits = np.unpackbits(frames[0][2][src], axis=1)
    pdesc = np.packbits(bits ^ (rng.random(bits.shape) < 0.07), axis=1)
    scales = (1.0, 1.7, 0.8, 1.2)
    Scw = np.stack([perturbed_scw(rng, scales[k % 4], *((0.08, 0.25) if far_every and k % far_every == far_every - 1 else (0.004, 0.01))) for k in range(n_kf)]) \
        if n_kf else np.zeros((0, 12), np.float32)
    return assemble(frames, [k % 2 for k in range(n_kf)], Scw, K4, sf, th, Xw, normal, dmin, dmax, pdesc)


PROFILE_SIZES = {"loop": (30, 2000), "merge_1_agent": (500, 3000), "merge_4_agents": (1000, 5000)}


def profile_scene(name: str, seed: int = 0) -> Scene:
    """The three sizes of scripts/fuse_sim3_profile.py: keyframes x points with about 1 000 features per keyframe"""
    n_kf, n_pts = PROFILE_SIZES[name]
    return make_scene(n_kf, n_pts, 1000, seed)
