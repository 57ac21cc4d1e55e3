"""The two projected searches of LoopFinder::ComputeSim3 / MapMatcher::ComputeSim3 on keyframes of a keyframe store:
ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (cslam/src/ORBmatcher.cpp:308-446) and ORBmatcher::SearchBySim3 (:1124-1348).

project_eval_resident / pair_eval_resident run ccm_sim3_project_eval_resident / ccm_sim3_pair_eval_resident; the *_resident_host forms evaluate the same pairs on the
store's shadows and project_eval_host / pair_eval_host on flat keyframe arrays, all through csrc/fuse_math.h compiled for the host (libccm_host.so).  derive is
ssm_derive (sR12, sR21, t21 of s12, R12, t12).  Sim3ProjectionSearch and search_by_sim3 are the host mirrors cslam::Sim3ProjectionSearch and
cslam::SearchBySim3Batch.

The keyframes, the Sim3s, the level table and the points of the projection search travel as a fuse_sim3.Scene plus one mask per keyframe; PairScene holds what the
pair search adds: points without normals and the job list.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional, Sequence

import numpy as np

from . import fuse_sim3 as fs, synth
from ._lib import CcmError, Context, _p, check, host, lib
from .fuse_sim3 import _c
from .kfstore import KeyFrameStore, _keys

STATUS = ("behind the camera", "outside the image", "distance range", "(unused)", "window empty", "no candidate at the level", "best distance > TH_HIGH", "hit")
TH_HIGH = 100


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    V, I, F = C.c_void_p, C.c_int, C.c_float
    kf = [I] + [V] * 7
    h.ccmh_sim3_project_eval_host.argtypes = kf + [V, V, V, I, V, F, F, I] + [V] * 5 + [V] * 4
    h.ccmh_sim3_pair_eval_host.argtypes = kf + [I, V, F, F, I] + [V] * 4 + [I] + [V] * 6 + [V] * 4
    h.ccmh_sim3_project_eval_resident_host.argtypes = [V, I, V, V, V, V, I, V, F, F, I] + [V] * 5 + [V] * 4
    h.ccmh_sim3_pair_eval_resident_host.argtypes = [V, I, V, I, V, F, F, I] + [V] * 4 + [I] + [V] * 6 + [V] * 4
    h.ccmh_ssm_derive.restype = None
    h.ccmh_ssm_derive.argtypes = [F] + [V] * 5
    h.ccmh_sim3_project_create.restype = V
    h.ccmh_sim3_project_create.argtypes = [V, I, C.c_int64, V, V, I, V, F, F, I] + [V] * 5
    h.ccmh_sim3_project_table.argtypes = [V] * 4
    h.ccmh_sim3_project_resolve.argtypes = [V, V, V, I, V, I, V, V]
    h.ccmh_sim3_project_n_reeval.restype = C.c_longlong
    h.ccmh_sim3_project_n_reeval.argtypes = [V]
    h.ccmh_sim3_project_destroy.restype = None
    h.ccmh_sim3_project_destroy.argtypes = [V]
    side = [I] + [V] * 6
    h.ccmh_search_by_sim3_resident.argtypes = [V, I, C.c_int64, C.c_int64] + side + side + [F, V, V, V, I, V, F, F] + [V] * 5
    return h


@functools.lru_cache(maxsize=None)
def _dev():
    l = lib()
    V, I, F = C.c_void_p, C.c_int, C.c_float
    l.ccm_sim3_project_eval_resident.argtypes = [V, V, I, V, V, V, V, I, V, F, F, I] + [V] * 5 + [V] * 4
    l.ccm_sim3_pair_eval_resident.argtypes = [V, V, I, V, I, V, F, F, I] + [V] * 4 + [I] + [V] * 6 + [V] * 4
    return l


def derive(s12: float, R12, t12):
    """ORBmatcher.cpp:1141-1143 as csrc/fuse_math.h states it: (sR12 (9), sR21 (9), t21 (3)) in f32"""
    R = _c(R12, np.float32, 9); t = _c(t12, np.float32, 3)
    a, b, c = np.zeros(9, np.float32), np.zeros(9, np.float32), np.zeros(3, np.float32)
    _host().ccmh_ssm_derive(C.c_float(s12), _p(R), _p(t), _p(a), _p(b), _p(c))
    return a, b, c


def pack_masks(masks: Sequence, counts: Sequence[int]):
    """(skip_off[K + 1], feat_skip) of one mask per keyframe; None stands for an all-zero mask of the keyframe's feature count"""
    m = [np.zeros(int(n), np.uint8) if x is None else np.ascontiguousarray(np.asarray(x, np.uint8).reshape(-1)) for x, n in zip(masks, counts)]
    off = np.zeros(len(m) + 1, np.int32)
    off[1:] = np.cumsum([x.size for x in m])
    return off, (np.concatenate(m) if m else np.zeros(0, np.uint8))


def _feature_counts(s: fs.Scene):
    return np.diff(s.feat_off[:s.K + 1]).tolist() if s.K else []


def _project_tail(s: fs.Scene):
    return [s.nlevels, _p(s.scale_factors), C.c_float(s.log_sf), C.c_float(s.th), s.P, _p(s.pos), _p(s.normal), _p(s.min_dist), _p(s.max_dist), _p(s.pt_desc)]


def project_eval_host(s: fs.Scene, masks=None, want_uv: bool = False, skip=None) -> dict:
    """every (keyframe, point) pair of `s` under the masks (one per keyframe, default all zero) on the calling thread; skip = (skip_off, feat_skip) passes raw arrays"""
    off, sk = skip if skip is not None else pack_masks(masks if masks is not None else [None] * s.K, _feature_counts(s))
    sh = _Shape(s.K, s.P)
    table, nv, nh, uv = fs._outputs(sh, want_uv)
    a = s.args()
    if _host().ccmh_sim3_project_eval_host(*a[:9], _p(off), _p(sk), *a[9:], _p(table), _p(nv), _p(nh), _p(uv)) != 0:
        raise CcmError("ccmh_sim3_project_eval_host: bad arguments")
    return fs._result(sh, table, nv, nh, uv)


def _resident_project(keys, s: fs.Scene, masks, counts, skip):
    keys = _keys(keys)
    if s.Scw.size != 12 * keys.size:
        raise ValueError("one Scw per key")
    off, sk = skip if skip is not None else pack_masks(masks if masks is not None else [None] * keys.size, counts)
    sh = _Shape(int(keys.size), s.P)
    return keys, off, sk, sh, [int(keys.size), _p(keys), _p(s.Scw), _p(off), _p(sk)] + _project_tail(s)


class _Shape:
    """K and P as fuse_sim3._outputs / _result read them (never negative: a refused call's outputs are empty)"""

    def __init__(self, K, P):
        self.K, self.P = max(int(K), 0), max(int(P), 0)


def _store_counts(store, keys, masks, skip):
    """the feature counts of the keys, read from the store where a default mask needs them"""
    if skip is not None or (masks is not None and not any(m is None for m in masks)):
        return [0] * len(_keys(keys))
    return [store.get(int(k), shadow=True)["n"] for k in _keys(keys)]


def project_eval_resident(ctx: Context, store: KeyFrameStore, keys, s: fs.Scene, masks=None, want_uv: bool = False, skip=None) -> dict:
    """ccm_sim3_project_eval_resident on the live keys `keys` with the Scw, the level table and the points of `s`; masks: one per key (None: all zero)"""
    counts = _store_counts(store, keys, masks, skip)
    keys, off, sk, sh, args = _resident_project(keys, s, masks, counts, skip)
    table, nv, nh, uv = fs._outputs(sh, want_uv)
    check(_dev().ccm_sim3_project_eval_resident(ctx.handle, store.raw, *args, _p(table), _p(nv), _p(nh), _p(uv)), ctx.handle)
    return fs._result(sh, table, nv, nh, uv)


def project_eval_resident_host(store: KeyFrameStore, keys, s: fs.Scene, masks=None, want_uv: bool = False, skip=None) -> dict:
    counts = _store_counts(store, keys, masks, skip)
    keys, off, sk, sh, args = _resident_project(keys, s, masks, counts, skip)
    table, nv, nh, uv = fs._outputs(sh, want_uv)
    if _host().ccmh_sim3_project_eval_resident_host(store.handle, *args, _p(table), _p(nv), _p(nh), _p(uv)) != 0:
        raise CcmError("ccmh_sim3_project_eval_resident_host: bad arguments or a key that is not live")
    return fs._result(sh, table, nv, nh, uv)


class PairScene:
    """The arguments of ccm_sim3_pair_eval_resident after the keys: the level table, points without normals and the jobs.  kfs: a fuse_sim3.Scene whose keyframes
    the flat host evaluator reads (its Scw and points are not read).  A job is (keyframe, K4 (4), source pose R t (12), transform sR t (12), first point, points)."""

    def __init__(self, kfs: fs.Scene, th, pos, min_dist, max_dist, pt_desc, jobs=()):
        self.kfs = kfs
        self.scale_factors = kfs.scale_factors; self.nlevels = kfs.nlevels; self.log_sf = kfs.log_sf; self.th = float(th)
        self.pos = _c(pos, np.float32); self.P = P = self.pos.size // 3
        self.min_dist = _c(min_dist, np.float32, P); self.max_dist = _c(max_dist, np.float32, P); self.pt_desc = _c(pt_desc, np.uint8, 32 * P)
        self.set_jobs(jobs)

    def set_jobs(self, jobs):
        jobs = list(jobs)
        self.J = J = len(jobs)
        self.job_kf = np.array([j[0] for j in jobs], np.int32)
        self.job_K4 = _c([j[1] for j in jobs] if J else [], np.float32, 4 * J)
        self.job_src = _c([j[2] for j in jobs] if J else [], np.float32, 12 * J)
        self.job_T = _c([j[3] for j in jobs] if J else [], np.float32, 12 * J)
        self.job_pt0 = np.array([j[4] for j in jobs], np.int32)
        self.job_n = np.array([j[5] for j in jobs], np.int32)
        self.total = int(np.clip(self.job_n, 0, None).sum()) if J else 0
        return self

    def tail(self):
        return [self.nlevels, _p(self.scale_factors), C.c_float(self.log_sf), C.c_float(self.th), self.P, _p(self.pos), _p(self.min_dist), _p(self.max_dist),
                _p(self.pt_desc), self.J, _p(self.job_kf), _p(self.job_K4), _p(self.job_src), _p(self.job_T), _p(self.job_pt0), _p(self.job_n)]

    def outputs(self, want_uv: bool):
        J = max(self.J, 0)
        return (np.zeros(self.total, np.uint32), np.zeros(J, np.int32), np.zeros(J, np.int32), np.zeros(2 * self.total, np.float32) if want_uv else None)

    def result(self, table, nv, nh, uv):
        out = dict(table=table, n_valid=nv, n_hit=nh, off=np.concatenate([[0], np.cumsum(np.clip(self.job_n, 0, None))]).astype(np.int64))
        if uv is not None:
            out["uv"] = uv.reshape(-1, 2)
        return out


def pair_eval_host(s: PairScene, want_uv: bool = False) -> dict:
    """every pair of the jobs of `s` against the keyframes of s.kfs on the calling thread; table: the jobs' words one after the other, off[j] = job j's first"""
    table, nv, nh, uv = s.outputs(want_uv)
    if _host().ccmh_sim3_pair_eval_host(*s.kfs.args()[:8], *s.tail(), _p(table), _p(nv), _p(nh), _p(uv)) != 0:
        raise CcmError("ccmh_sim3_pair_eval_host: bad arguments")
    return s.result(table, nv, nh, uv)


def pair_eval_resident(ctx: Context, store: KeyFrameStore, keys, s: PairScene, want_uv: bool = False) -> dict:
    """ccm_sim3_pair_eval_resident on the live keys `keys` (job_kf indexes them)"""
    keys = _keys(keys)
    table, nv, nh, uv = s.outputs(want_uv)
    check(_dev().ccm_sim3_pair_eval_resident(ctx.handle, store.raw, int(keys.size), _p(keys), *s.tail(), _p(table), _p(nv), _p(nh), _p(uv)), ctx.handle)
    return s.result(table, nv, nh, uv)


def pair_eval_resident_host(store: KeyFrameStore, keys, s: PairScene, want_uv: bool = False) -> dict:
    keys = _keys(keys)
    table, nv, nh, uv = s.outputs(want_uv)
    if _host().ccmh_sim3_pair_eval_resident_host(store.handle, int(keys.size), _p(keys), *s.tail(), _p(table), _p(nv), _p(nh), _p(uv)) != 0:
        raise CcmError("ccmh_sim3_pair_eval_resident_host: bad arguments or a key that is not live")
    return s.result(table, nv, nh, uv)


class Sim3ProjectionSearch:
    """cslam::Sim3ProjectionSearch on one live key: ONE evaluation of every point against the initial mask at construction (on the store's device, or with
    host=True / a host-only store on the calling thread), then resolve(...) replays the reference's loop.  `s`: a fuse_sim3.Scene with one Scw and the points."""

    def __init__(self, store: KeyFrameStore, key: int, s: fs.Scene, matched0, host: bool = False):
        if s.Scw.size != 12:
            raise ValueError("one Scw")
        self.P = s.P
        m0 = np.ascontiguousarray(np.asarray(matched0, np.uint8).reshape(-1))
        self.N = int(m0.size)
        self._h = _host().ccmh_sim3_project_create(store.handle, -1 if host else store.device, int(key), _p(s.Scw), _p(m0), *_project_tail(s))
        if not self._h:
            raise CcmError("ccmh_sim3_project_create failed (bad arguments, a key that is not live or a device error)")

    def table(self) -> dict:
        table = np.zeros(self.P, np.uint32); nv, nh = C.c_int32(), C.c_int32()
        _host().ccmh_sim3_project_table(self._h, _p(table), C.byref(nv), C.byref(nh))
        return dict(table=table, n_valid=nv.value, n_hit=nh.value)

    def resolve(self, matched, skip_now=None, existing_idx=None):
        """(nmatches, matched (N, updated copy), bestIdx[P], remap[P]); matched: >= 0 where vpMatched is set on entry"""
        m = np.ascontiguousarray(np.asarray(matched, np.int32).reshape(-1)).copy()
        if m.size != self.N:
            raise ValueError("matched: one entry per feature")
        skip = _c(skip_now, np.uint8, self.P) if skip_now is not None else None
        ex = _c(existing_idx, np.int32, self.P) if existing_idx is not None else None
        bi = np.zeros(self.P, np.int32); rm = np.zeros(self.P, np.int32)
        n = _host().ccmh_sim3_project_resolve(self._h, _p(skip), _p(ex), self.N, _p(m), self.P, _p(bi), _p(rm))
        if n < 0:
            raise CcmError(f"ccmh_sim3_project_resolve: {n}")
        return n, m, bi, rm

    def n_reeval(self) -> int:
        return int(_host().ccmh_sim3_project_n_reeval(self._h))

    def close(self):
        if self._h:
            _host().ccmh_sim3_project_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Side:
    """one keyframe of SearchBySim3: per feature slot live (pMP && !isBad()), position, bounds and descriptor of its point, and the keyframe's pose R (9), t (3)"""

    def __init__(self, live, pos, min_dist, max_dist, desc, pose12):
        self.live = np.ascontiguousarray(np.asarray(live, np.uint8).reshape(-1)); self.N = N = int(self.live.size)
        self.pos = _c(pos, np.float32, 3 * N); self.min_dist = _c(min_dist, np.float32, N); self.max_dist = _c(max_dist, np.float32, N)
        self.desc = _c(desc, np.uint8, 32 * N); self.pose = _c(pose12, np.float32, 12)

    def args(self):
        return [self.N, _p(self.live), _p(self.pos), _p(self.min_dist), _p(self.max_dist), _p(self.desc), _p(self.pose)]


def pose12(T):
    """R (9, row-major), t (3) of a 4 x 4 (or 3 x 4) pose"""
    T = np.asarray(T, np.float32).reshape(-1, 4)
    return np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]).astype(np.float32)


def search_by_sim3(store: KeyFrameStore, key1: int, key2: int, side1: Side, side2: Side, s12: float, R12, t12, matches12_in, scale_factors, th: float,
                   host: bool = False, log_sf: Optional[float] = None) -> dict:
    """cslam::SearchBySim3Batch: nFound, matches12 (N1), vnMatch1 (N1), vnMatch2 (N2), n_valid / n_hit per direction.  log_sf: mfLogScaleFactor where the caller
    has it (default: fuse_sim3.log_scale_factor of the table)"""
    sf = _c(scale_factors, np.float32)
    log_sf = fs.log_scale_factor(sf) if log_sf is None else float(log_sf)
    R = _c(R12, np.float32, 9); t = _c(t12, np.float32, 3)
    m_in = _c(matches12_in, np.int32, side1.N)
    m = np.zeros(side1.N, np.int32); v1 = np.zeros(side1.N, np.int32); v2 = np.zeros(side2.N, np.int32); nv = np.zeros(2, np.int32); nh = np.zeros(2, np.int32)
    n = _host().ccmh_search_by_sim3_resident(store.handle, -1 if host else store.device, int(key1), int(key2), *side1.args(), *side2.args(), C.c_float(s12), _p(R), _p(t),
                                             _p(m_in), int(sf.size), _p(sf), C.c_float(log_sf), C.c_float(th), _p(m), _p(v1), _p(v2), _p(nv), _p(nh))
    if n < 0:
        raise CcmError(f"ccmh_search_by_sim3_resident: {n}")
    return dict(nFound=n, matches12=m, vnMatch1=v1, vnMatch2=v2, n_valid=nv, n_hit=nh)


def single_keyframe_scene(xy, octave, desc, K4, bounds, Scw12, scale_factors, th, pos, normal, min_dist, max_dist, pt_desc) -> fs.Scene:
    """a fuse_sim3.Scene of one keyframe with the caller's grid (fuse_sim3.build_grid: the reference's order)"""
    return fs.assemble([(np.asarray(xy, np.float32).reshape(-1, 2), np.asarray(octave, np.uint8), np.asarray(desc, np.uint8).reshape(-1, 32))], [0],
                       np.asarray(Scw12, np.float32).reshape(1, 12), K4, scale_factors, th, pos, normal, min_dist, max_dist, pt_desc, bounds)


def keyframes_scene(frames, K4, bounds, scale_factors, th=1.0) -> fs.Scene:
    """a fuse_sim3.Scene that holds keyframes alone (identity Sim3s, no points), one per entry of frames = [(xy, octave, desc)]: what PairScene and
    KeyFrameStore.add_scene read"""
    K = len(frames)
    Scw = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (K, 1))
    z = np.zeros(0, np.float32)
    return fs.assemble([(np.asarray(f[0], np.float32).reshape(-1, 2), np.asarray(f[1], np.uint8), np.asarray(f[2], np.uint8).reshape(-1, 32)) for f in frames],
                       list(range(K)), Scw, K4, scale_factors, th, z, z, z, z, np.zeros(0, np.uint8), bounds)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# generators (numpy only; nothing here touches the device)
# ---------------------------------------------------------------------------------------------------------------------------------------------
PROFILE_SIZES = {"loop": dict(points=8000, live=800), "small": dict(points=2000, live=300)}


def projection_profile_scene(n_pts: int, n_feat: int = 1000, seed: int = 0, th: float = 10.0, matched_share: float = 0.1):
    """(Scene, matched0): one keyframe of n_feat features against n_pts loop points (fuse_sim3.make_scene), a tenth of the features matched on entry"""
    sc = fs.make_scene(1, n_pts, n_feat, seed, th=th, far_every=0)
    rng = np.random.default_rng(seed + 1)
    return sc, (rng.random(n_feat) < matched_share).astype(np.uint8)


def pair_profile_scene(n_live: int, n_feat: int = 1000, seed: int = 0, th: float = 7.5) -> dict:
    """Two keyframes of n_feat features that see one scene through a similarity (s12, R12, t12), n_live of each keyframe's slots holding a point, a few matches on
    entry: kfs (the keyframes as a Scene), side1, side2, s12, R12, t12, matches12_in, th — the arguments of search_by_sim3"""
    rng = np.random.default_rng(seed)
    sf = synth.scale_tables()[0]
    K4 = np.array(synth.EUROC_K, np.float64)
    xy1 = np.stack([rng.uniform(24, synth.IMG_W - 24, n_feat), rng.uniform(24, synth.IMG_H - 24, n_feat)], 1)
    oc1 = np.minimum(rng.geometric(0.35, n_feat) - 1, 7).astype(np.uint8)
    d1 = rng.integers(0, 256, (n_feat, 32), dtype=np.uint8)
    s12 = 1.15
    R12 = synth.rodrigues(np.array([[0.006, 0.03, 0.003]]))[0]; t12 = np.array([0.05, -0.02, 0.1])
    sR21 = R12.T / s12; t21 = -sR21 @ t12
    z = rng.uniform(3, 9, n_feat)
    Xc1 = np.stack([(xy1[:, 0] - K4[2]) / K4[0] * z, (xy1[:, 1] - K4[3]) / K4[1] * z, z], 1)
    Xc2 = Xc1 @ sR21.T + t21
    perm = rng.permutation(n_feat)
    uv2 = np.stack([K4[0] * Xc2[:, 0] / Xc2[:, 2] + K4[2], K4[1] * Xc2[:, 1] / Xc2[:, 2] + K4[3]], 1) + rng.normal(0, 1.0, (n_feat, 2))
    out = (uv2[:, 0] < 24) | (uv2[:, 0] > synth.IMG_W - 24) | (uv2[:, 1] < 24) | (uv2[:, 1] > synth.IMG_H - 24)
    uv2[out] = np.stack([rng.uniform(24, synth.IMG_W - 24, out.sum()), rng.uniform(24, synth.IMG_H - 24, out.sum())], 1)
    xy2 = uv2[perm]; oc2 = oc1[perm]
    flip = lambda d, p: np.packbits(np.unpackbits(d, axis=1) ^ (rng.random((d.shape[0], 256)) < p), axis=1)
    d2 = flip(d1, 0.06)[perm]
    Xc2p = np.stack([(xy2[:, 0] - K4[2]) / K4[0], (xy2[:, 1] - K4[3]) / K4[1], np.ones(n_feat)], 1) * Xc2[perm][:, 2:3]
    dist1 = np.linalg.norm(Xc2, axis=1); dist2 = np.linalg.norm(Xc2p @ (s12 * R12).T + t12, axis=1)
    dmax1 = dist1 * 1.2 ** (np.clip(oc1.astype(int) + rng.integers(0, 2, n_feat), 0, 7) - 0.5)
    dmax2 = dist2 * 1.2 ** (np.clip(oc2.astype(int) + rng.integers(0, 2, n_feat), 0, 7) - 0.5)
    live = lambda: (rng.permutation(n_feat) < n_live).astype(np.uint8)
    ident = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)        # both maps are written in their own camera's frame
    side1 = Side(live(), Xc1, dmax1 / 1.2 ** 7, dmax1, flip(d1, 0.03), ident)
    side2 = Side(live(), Xc2p, dmax2 / 1.2 ** 7, dmax2, flip(d2, 0.03), ident)
    inv = np.empty(n_feat, np.int64); inv[perm] = np.arange(n_feat)
    m_in = -np.ones(n_feat, np.int32)
    both = np.flatnonzero((side1.live > 0) & (side2.live[inv] > 0))
    pre = rng.choice(both, min(both.size, max(n_live // 15, 1)), replace=False)
    m_in[pre] = inv[pre]
    kfs = keyframes_scene([(xy1, oc1, d1), (xy2, oc2, d2)], K4.astype(np.float32), fs.BOUNDS, sf)
    return dict(kfs=kfs, side1=side1, side2=side2, s12=s12, R12=R12.astype(np.float32), t12=t12.astype(np.float32), matches12_in=m_in, th=th, true12=inv)
