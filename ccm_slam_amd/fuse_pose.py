"""LocalMapping::SearchInNeighbors (cslam/src/Mapping.cpp:471-547): ORBmatcher::Fuse(pKF, vpMapPoints, th = 3) (ORBmatcher.cpp:854-993) for every fuse target
with the current keyframe's points, then once on the current keyframe with the targets' points.  Both directions are one job list.

fuse_pose_eval runs ccm_fuse_pose_eval (every pair of every job in one launch), fuse_pose_eval_host the same lines compiled for the host (libccm_host.so);
unpack_table (fuse_sim3's) splits the packed answers.  SearchInNeighborsBatch is the host mirror cslam::SearchInNeighborsBatch: resolve(c, ...) answers the c-th
Fuse call of the first loop, resolve_current(...) the call on the current keyframe.

make_scene / profile_scene generate keyframes, points and jobs as numpy arrays; nothing in them touches the device.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional, Sequence

import numpy as np

from . import synth
from ._lib import CcmError, Context, _p, check, host, lib
from .fuse_sim3 import (BOUNDS, CELLS, GRID_COLS, GRID_ROWS, NO_DIST, NO_IDX, _c, _rot_y, build_grid, kf_record, log_scale_factor, unpack_table)  # noqa: F401
from .sim3_correct import camera_center

STATUS = ("behind the camera", "outside the image", "distance range", "viewing angle", "window empty", "no candidate passed the level filter and the chi2 gate",
          "best distance > TH_LOW", "hit")
TH = 3.0      # Mapping.cpp: matcher.Fuse(pKFi, vpMapPointMatches) with the default th = 3.0

# the arguments of ccm_fuse_pose_eval after the context, up to the outputs
_EV = [C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_int] + [C.c_void_p] * 5
_JOBS = [C.c_int] + [C.c_void_p] * 3


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    V = C.c_void_p
    h.ccmh_fuse_pose_create.restype = V
    h.ccmh_fuse_pose_create.argtypes = [C.c_int] + _EV + [C.c_int, V, C.c_int, C.c_int]
    h.ccmh_fuse_pose_table.argtypes = [V] * 4
    h.ccmh_fuse_pose_resolve.argtypes = [V, C.c_int, V, V, C.c_int, V, V]
    h.ccmh_fuse_pose_resolve_current.argtypes = [V, C.c_int] + [V] * 10
    for f in (h.ccmh_fuse_pose_n_reeval, h.ccmh_fuse_pose_n_unpredicted):
        f.argtypes = [V]
        f.restype = C.c_longlong
    h.ccmh_fuse_pose_destroy.argtypes = [V]
    h.ccmh_fuse_pose_destroy.restype = None
    h.ccmh_fuse_pose_eval_host.argtypes = _EV + _JOBS + [V] * 5
    return h


@functools.lru_cache(maxsize=None)
def _dev():
    l = lib()
    l.ccm_fuse_pose_eval.argtypes = [C.c_void_p] + _EV + _JOBS + [C.c_void_p] * 4
    return l


def pose_record(T) -> np.ndarray:
    """pose[15] per keyframe from Tcw (n, 4, 4) or (n, 12): GetRotation() (row-major), GetTranslation() and GetCameraCenter() as KeyFrame::SetPose leaves them
    (Ow through the project's restatement, sim3_correct.camera_center / csrc/gba_apply_math.h)"""
    T = np.asarray(T, np.float32)
    four = T.shape[-1] == 16 or (T.ndim >= 2 and T.shape[-2:] == (4, 4))
    T = np.ascontiguousarray(T.reshape(-1, 4, 4)[:, :3, :] if four else T.reshape(-1, 3, 4))
    out = np.zeros((T.shape[0], 15), np.float32)
    out[:, :9] = T[:, :, :3].reshape(-1, 9)
    out[:, 9:12] = T[:, :, 3]
    out[:, 12:] = camera_center(T.reshape(-1, 12))
    return out


class Scene:
    """The flat arguments of ccm_fuse_pose_eval, checked for their lengths only (the values are the library's to check)"""

    def __init__(self, rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off, cell_idx, pose, scale_factors, inv_sigma2, log_sf, th, pos, normal, min_dist, max_dist,
                 pt_desc, jobs=()):
        self.feat_off = _c(feat_off, np.int32)
        self.K = K = max(self.feat_off.size - 1, 0) if rec is not None and np.size(rec) else 0
        F = int(self.feat_off[K]) if K and 0 <= int(self.feat_off[K]) < (1 << 31) else 0
        self.rec = _c(rec, np.float32, 10 * K)
        self.feat_xy = _c(feat_xy, np.float32); self.feat_octave = _c(feat_octave, np.uint8); self.feat_desc = _c(feat_desc, np.uint8)
        self.cell_off = _c(cell_off, np.int32, (CELLS + 1) * K); self.cell_idx = _c(cell_idx, np.int32)
        if self.feat_xy.size < 2 * F or self.feat_octave.size < F or self.feat_desc.size < 32 * F or self.cell_idx.size < F:
            raise ValueError("feature arrays shorter than feat_off says")
        self.pose = _c(pose, np.float32, 15 * K)
        self.scale_factors = _c(scale_factors, np.float32); self.nlevels = int(self.scale_factors.size)
        self.inv_sigma2 = _c(inv_sigma2, np.float32, self.nlevels)
        self.log_sf = float(log_sf); self.th = float(th)
        self.pos = _c(pos, np.float32); self.P = P = self.pos.size // 3
        self.normal = _c(normal, np.float32, 3 * P); self.min_dist = _c(min_dist, np.float32, P); self.max_dist = _c(max_dist, np.float32, P)
        self.pt_desc = _c(pt_desc, np.uint8, 32 * P)
        self.set_jobs(jobs)

    def set_jobs(self, jobs):
        """jobs: [(keyframe, first point, points)]"""
        j = np.asarray(list(jobs), np.int64).reshape(-1, 3)
        self.J = int(j.shape[0])
        self.job_kf = np.ascontiguousarray(j[:, 0], np.int32); self.job_pt0 = np.ascontiguousarray(j[:, 1], np.int32); self.job_n = np.ascontiguousarray(j[:, 2], np.int32)

    @property
    def jobs(self):
        return [(int(a), int(b), int(c)) for a, b, c in zip(self.job_kf, self.job_pt0, self.job_n)]

    @property
    def job_off(self) -> np.ndarray:
        """where each job's words start in the table; [J] is the table's length"""
        return np.concatenate([[0], np.cumsum(np.maximum(self.job_n.astype(np.int64), 0))])

    def args(self):
        return [self.K, _p(self.rec), _p(self.feat_off), _p(self.feat_xy), _p(self.feat_octave), _p(self.feat_desc), _p(self.cell_off), _p(self.cell_idx), _p(self.pose),
                self.nlevels, _p(self.scale_factors), _p(self.inv_sigma2), C.c_float(self.log_sf), C.c_float(self.th), self.P, _p(self.pos), _p(self.normal),
                _p(self.min_dist), _p(self.max_dist), _p(self.pt_desc)]

    def job_args(self):
        return [self.J, _p(self.job_kf), _p(self.job_pt0), _p(self.job_n)]

    def subset(self, kfs: Optional[Sequence[int]] = None, n_pts: Optional[int] = None, jobs=None) -> "Scene":
        """the keyframes `kfs` (in that order; None: all), the first n_pts points (None: all) and the jobs `jobs` (None: the scene's own, which then must fit;
        their keyframes count in the NEW order)"""
        P = self.P if n_pts is None else int(n_pts)
        kfs = list(range(self.K)) if kfs is None else list(kfs)
        off = [0]; xy = []; oc = []; de = []; ci = []
        for k in kfs:
            a, b = int(self.feat_off[k]), int(self.feat_off[k + 1])
            xy.append(self.feat_xy[2 * a:2 * b]); oc.append(self.feat_octave[a:b]); de.append(self.feat_desc[32 * a:32 * b]); ci.append(self.cell_idx[a:b])
            off.append(off[-1] + b - a)
        cat = lambda v, dt: np.concatenate(v) if v else np.zeros(0, dt)
        return Scene(self.rec.reshape(-1, 10)[kfs], off, cat(xy, np.float32), cat(oc, np.uint8), cat(de, np.uint8), self.cell_off.reshape(-1, CELLS + 1)[kfs],
                     cat(ci, np.int32), self.pose.reshape(-1, 15)[kfs], self.scale_factors, self.inv_sigma2, self.log_sf, self.th, self.pos[:3 * P], self.normal[:3 * P],
                     self.min_dist[:P], self.max_dist[:P], self.pt_desc[:32 * P], self.jobs if jobs is None else jobs)


def _outputs(s: Scene, want_uv: bool):
    n = int(s.job_off[-1])
    return (np.zeros(n, np.uint32), np.zeros(s.J, np.int32), np.zeros(s.J, np.int32), np.zeros(2 * n, np.float32) if want_uv else None)


def _result(s: Scene, table, n_valid, n_hit, uv, n_cand=None):
    out = dict(table=table, n_valid=n_valid, n_hit=n_hit, job_off=s.job_off)
    if uv is not None:
        out["uv"] = uv.reshape(-1, 2)
    if n_cand is not None:
        out["n_cand"] = n_cand
    return out


def job_rows(res: dict, j: int, key: str = "table"):
    """job j's part of a result's table (or uv, n_cand)"""
    return res[key][int(res["job_off"][j]):int(res["job_off"][j + 1])]


def fuse_pose_eval(ctx: Context, s: Scene, want_uv: bool = False) -> dict:
    """ccm_fuse_pose_eval: table (the jobs' words one after the other), n_valid[J], n_hit[J], job_off[J + 1] and, when asked for, uv (pairs, 2)"""
    table, nv, nh, uv = _outputs(s, want_uv)
    check(_dev().ccm_fuse_pose_eval(ctx.handle, *s.args(), *s.job_args(), _p(table), _p(nv), _p(nh), _p(uv)), ctx.handle)
    return _result(s, table, nv, nh, uv)


def fuse_pose_eval_host(s: Scene, want_uv: bool = False, want_cand: bool = False) -> dict:
    """The same through csrc/fuse_math.h on the calling thread; n_cand = the size of vIndices per pair when asked for"""
    table, nv, nh, uv = _outputs(s, want_uv)
    nc = np.zeros(table.size, np.int32) if want_cand else None
    if _host().ccmh_fuse_pose_eval_host(*s.args(), *s.job_args(), _p(table), _p(nv), _p(nh), _p(uv), _p(nc)) != 0:
        raise CcmError("ccmh_fuse_pose_eval_host: bad arguments")
    return _result(s, table, nv, nh, uv, nc)


class SearchInNeighborsBatch:
    """cslam::SearchInNeighborsBatch: ONE evaluation of both directions at construction (ctx = None: the host evaluator), then resolve(c, ...) per Fuse call of
    the first loop and resolve_current(...) for the call on the current keyframe.  The scene's first n_current points are the current keyframe's, the rest the
    predicted fuse candidates; targets[c] is the keyframe of call c and `current` the current keyframe (None: no second direction).  The scene's own jobs are
    not read."""

    def __init__(self, ctx: Optional[Context], s: Scene, targets, current: Optional[int], n_current: int, device: int = 0):
        self.scene = s
        self.targets = np.ascontiguousarray(targets, np.int32)
        self.C = int(self.targets.size); self.P1 = int(n_current); self.P2 = s.P - int(n_current)
        self.J = self.C + (current is not None)
        self._h = _host().ccmh_fuse_pose_create(-1 if ctx is None else int(getattr(ctx, "device", device)), *s.args(), self.C, _p(self.targets),
                                                -1 if current is None else int(current), self.P1)
        if not self._h:
            raise CcmError("ccmh_fuse_pose_create failed (bad arguments or a device error)")

    def table(self) -> dict:
        n = self.C * self.P1 + (self.P2 if self.J > self.C else 0)
        table = np.zeros(n, np.uint32); nv = np.zeros(self.J, np.int32); nh = np.zeros(self.J, np.int32)
        _host().ccmh_fuse_pose_table(self._h, _p(table), _p(nv), _p(nh))
        return dict(table=table, calls=table[:self.C * self.P1].reshape(self.C, self.P1), current=table[self.C * self.P1:], n_valid=nv, n_hit=nh)

    def resolve(self, c: int, skip_now=None, desc_now=None):
        """(nFused, bestIdx[P1] (-1: not fused), bestDist[P1]) of the c-th Fuse call of the first loop"""
        P = self.P1
        skip = _c(skip_now, np.uint8, P) if skip_now is not None else None
        desc = _c(desc_now, np.uint8, 32 * P) if desc_now is not None else None
        bi = np.zeros(P, np.int32); bd = np.zeros(P, np.int32)
        n = _host().ccmh_fuse_pose_resolve(self._h, int(c), _p(skip), _p(desc), P, _p(bi), _p(bd))
        if n < 0:
            raise CcmError(f"ccmh_fuse_pose_resolve: {n}")
        return n, bi, bd

    def resolve_current(self, slot, skip_now=None, desc_now=None, fresh=None):
        """(nFused, bestIdx[n], bestDist[n]) of Fuse(mpCurrentKeyFrame, vpFuseCandidates) for the n candidates of `slot`; fresh = (pos, normal, min_dist, max_dist,
        desc) with n entries each, read for the candidates with slot -1"""
        slot = np.ascontiguousarray(slot, np.int32); n = int(slot.size)
        skip = _c(skip_now, np.uint8, n) if skip_now is not None else None
        desc = _c(desc_now, np.uint8, 32 * n) if desc_now is not None else None
        fr = [None] * 5
        if fresh is not None:
            fr = [_c(fresh[0], np.float32, 3 * n), _c(fresh[1], np.float32, 3 * n), _c(fresh[2], np.float32, n), _c(fresh[3], np.float32, n), _c(fresh[4], np.uint8, 32 * n)]
        bi = np.zeros(n, np.int32); bd = np.zeros(n, np.int32)
        nf = _host().ccmh_fuse_pose_resolve_current(self._h, n, _p(slot), _p(skip), _p(desc), *[_p(a) for a in fr], _p(bi), _p(bd))
        if nf < 0:
            raise CcmError(f"ccmh_fuse_pose_resolve_current: {nf}")
        return nf, bi, bd

    def n_reeval(self) -> int:
        return int(_host().ccmh_fuse_pose_n_reeval(self._h))

    def n_unpredicted(self) -> int:
        return int(_host().ccmh_fuse_pose_n_unpredicted(self._h))

    def close(self):
        if self._h:
            _host().ccmh_fuse_pose_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------------------------
def perturbed_pose(rng, d_rad: float, d_m: float, ang: float = 0.3, t=(0.4, -0.2, 0.7)) -> np.ndarray:
    """Rows 0..2 of a Tcw around the pose of the scenes below, perturbed by d_rad about a random axis and d_m in translation"""
    R = synth.rodrigues((d_rad * rng.normal(size=3) / np.sqrt(3.0))[None])[0] @ _rot_y(ang)
    tt = np.asarray(t, np.float64) + d_m * rng.normal(size=3) / np.sqrt(3.0)
    return np.concatenate([R, tt[:, None]], 1).astype(np.float32).reshape(-1)


def assemble(frames, which, Tcw, K4, scale_factors, inv_sigma2, th, pos, normal, min_dist, max_dist, pt_desc, jobs=(), bounds=BOUNDS) -> Scene:
    """A Scene from per-frame features: frames = [(xy (n, 2), octave, desc (n, 32))], which[k] = the frame keyframe k shows, Tcw (K, 12) or (K, 4, 4)"""
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
    pose = pose_record(Tcw) if len(which) else np.zeros((0, 15), np.float32)
    return Scene(rec, off, cat(xy, np.float32), cat(oc, np.uint8), cat(de, np.uint8), cat(co, np.int32), cat(ci, np.int32), pose, scale_factors, inv_sigma2,
                 log_scale_factor(scale_factors), th, pos, normal, min_dist, max_dist, pt_desc, jobs)


def make_scene(n_calls: int, n_current: int, n_candidates: int, n_feat: int = 1000, seed: int = 0, th: float = TH, n_targets: Optional[int] = None) -> Scene:
    """A SearchInNeighbors: n_targets target keyframes (default n_calls: one call each, otherwise the calls cycle through them) and the current keyframe (the last
    one) around one pose, 0.004 rad and 0.01 m apart, alternating between two synthetic feature sets (n_feat keypoints each, octaves 0..7; the second is the first
    a few pixels on); n_current points back-projected from the first set with noisy copies of its descriptors, then n_candidates more of the same kind.
    Jobs: call c = (target, the first n_current points), then (current keyframe, the n_candidates others)."""
    rng = np.random.default_rng(seed)
    sf, _, _, isig = synth.scale_tables()
    K4 = np.array(synth.EUROC_K, np.float32)
    xy = np.stack([rng.uniform(24, synth.IMG_W - 24, n_feat), rng.uniform(24, synth.IMG_H - 24, n_feat)], 1).astype(np.float32)
    octv = np.minimum(rng.geometric(0.35, n_feat) - 1, 7).astype(np.uint8)
    desc = rng.integers(0, 256, (n_feat, 32), dtype=np.uint8)
    perm = rng.permutation(n_feat)
    xy2 = (xy[perm] + np.array([2.5, -1.5]) + rng.normal(0, 0.7, (n_feat, 2))).astype(np.float32)
    desc2 = np.packbits(np.unpackbits(desc[perm], axis=1) ^ (rng.random((n_feat, 256)) < 0.05), axis=1)
    frames = [(xy, octv, desc), (xy2, octv[perm], desc2)]
    R = _rot_y(0.3); t = np.array([0.4, -0.2, 0.7])
    n_pts = n_current + n_candidates
    src = rng.integers(0, n_feat, n_pts)
    z = rng.uniform(3, 9, n_pts)
    uu = xy[src, 0] + rng.normal(0, 1.0, n_pts); vv = xy[src, 1] + rng.normal(0, 1.0, n_pts)
    Xc = np.stack([(uu - K4[2]) / K4[0] * z, (vv - K4[3]) / K4[1] * z, z], 1)
    Xw = (Xc - t) @ R
    PO = Xw + R.T @ t
    dist = np.linalg.norm(PO, axis=1)
    normal = PO / dist[:, None]
    lvl = np.clip(octv[src].astype(int) + rng.integers(0, 2, n_pts), 0, 7)
    dmax = dist * 1.2 ** (lvl - 0.5)
    dmin = dmax / 1.2 ** 7
    bits = np.unpackbits(desc[src], axis=1)
    pdesc = np.packbits(bits ^ (rng.random(bits.shape) < 0.07), axis=1)
    T = n_calls if n_targets is None else n_targets
    Tcw = np.stack([perturbed_pose(rng, 0.004, 0.01) for _ in range(T + 1)])
    jobs = [(c % T, 0, n_current) for c in range(n_calls)] + [(T, n_current, n_candidates)]
    return assemble(frames, [k % 2 for k in range(T + 1)], Tcw, K4, sf, isig, th, Xw, normal, dmin, dmax, pdesc, jobs)


# calls x the current keyframe's points + candidates: an agent's keyframe, a server keyframe in a merged map, a small one
PROFILE_SIZES = {"agent": (25, 1000, 8000), "server_merged": (100, 1000, 25000), "small": (5, 300, 1000)}


def profile_scene(name: str, seed: int = 0) -> Scene:
    """The three rows of scripts/fuse_pose_profile.py, about 1 000 features per keyframe"""
    c, p1, p2 = PROFILE_SIZES[name]
    return make_scene(c, p1, p2, 1000, seed)
