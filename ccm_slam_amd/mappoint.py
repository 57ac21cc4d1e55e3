"""MapPoint::ComputeDistinctiveDescriptors (cslam/src/MapPoint.cpp:929-994) and MapPoint::UpdateNormalAndDepth (:779-823) for the map points a map stage touched,
on keyframes of a keyframe store.

refresh_resident runs ccm_mappoint_refresh_resident: ONE upload, ONE launch and one download for P points given as flat observation lists (index into keys, feature
index).  refresh_host evaluates the same call on the store's shadows through csrc/mappoint_math.h compiled for the host (libccm_host.so).  Both return best_obs,
best_desc, normal, min_dist, max_dist and status per point.  Refresh is the host mirror cslam::MapPointRefresh.  profile_scene builds the workloads of
scripts/mappoint_refresh_profile.py.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

import numpy as np

from . import fuse_sim3 as fs
from ._lib import CcmError, Context, _p, check, host, lib
from .kfstore import KeyFrameStore

# status[p] (csrc/mappoint_math.h)
DESC, NORMAL_DEPTH, OCTAVE_BEYOND = 1, 2, 4
MAX_OBS = 256


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    V, I = C.c_void_p, C.c_int
    h.ccmh_mappoint_refresh_eval_resident_host.argtypes = [V, I, V, V, I] + [V] * 6 + [I] + [V] * 7
    h.ccmh_mappoint_refresh_create.restype = V
    h.ccmh_mappoint_refresh_create.argtypes = [V, I, I, V, V, I] + [V] * 9 + [I, V]
    h.ccmh_mappoint_refresh_result.argtypes = [V, I] + [V] * 7
    h.ccmh_mappoint_refresh_destroy.restype = None
    h.ccmh_mappoint_refresh_destroy.argtypes = [V]
    return h


@functools.lru_cache(maxsize=None)
def _dev():
    l = lib()
    V, I = C.c_void_p, C.c_int
    l.ccm_mappoint_refresh_resident.argtypes = [V, V, I, V, V, I] + [V] * 6 + [I] + [V] * 7
    return l


_IN_TYPES = (np.int64, np.float32, np.int32, np.int32, np.int32, np.float32, np.int32, np.int32, np.float32)


def _inputs(keys, kf_center, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, scale_factors):
    """the nine input arrays, contiguous and typed (None: a null pointer)"""
    return [None if x is None else np.ascontiguousarray(np.asarray(x, dt).reshape(-1)) for x, dt in
            zip((keys, kf_center, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, scale_factors), _IN_TYPES)]


def _outputs(P, normal, min_dist, max_dist, want_desc):
    seed = lambda x, n: np.zeros(n, np.float32) if x is None else np.array(x, np.float32).reshape(-1).copy()
    return dict(best_obs=np.full(P, -1, np.int32), best_desc=np.zeros((P, 32), np.uint8) if want_desc else None, normal=seed(normal, 3 * P),
                min_dist=seed(min_dist, P), max_dist=seed(max_dist, P), status=np.zeros(P, np.uint8))


def _call(fn, first, a, P, nlevels, out):
    keys, ctr, off, okf, ofeat, pos, rkf, rfeat, sf = a
    return int(fn(*first, 0 if keys is None else int(keys.size), _p(keys), _p(ctr), int(P), _p(off), _p(okf), _p(ofeat), _p(pos), _p(rkf), _p(rfeat), int(nlevels), _p(sf),
                  _p(out["best_obs"]), _p(out["best_desc"]), _p(out["normal"]), _p(out["min_dist"]), _p(out["max_dist"]), _p(out["status"])))


def _result(out, P):
    out["normal"] = out["normal"].reshape(P, 3)
    return out


def refresh_resident(ctx: Context, store: KeyFrameStore, keys, kf_center, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, scale_factors, normal=None, min_dist=None,
                     max_dist=None, want_desc: bool = True) -> dict:
    """ccm_mappoint_refresh_resident; normal / min_dist / max_dist: the points' current values (default zeros), which come back where a point keeps them"""
    a = _inputs(keys, kf_center, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, scale_factors)
    P = int(a[2].size) - 1
    out = _outputs(P, normal, min_dist, max_dist, want_desc)
    check(_call(_dev().ccm_mappoint_refresh_resident, (ctx.handle, store.raw), a, P, a[8].size, out), ctx.handle)
    return _result(out, P)


def refresh_host(store: KeyFrameStore, keys, kf_center, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, scale_factors, normal=None, min_dist=None, max_dist=None,
                 want_desc: bool = True) -> dict:
    """the same call on the store's shadows on the calling thread (mappoint_refresh_eval_host of csrc/mappoint_math.h)"""
    a = _inputs(keys, kf_center, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, scale_factors)
    P = int(a[2].size) - 1
    out = _outputs(P, normal, min_dist, max_dist, want_desc)
    if _call(_host().ccmh_mappoint_refresh_eval_resident_host, (store.handle,), a, P, a[8].size, out) != 0:
        raise CcmError("ccmh_mappoint_refresh_eval_resident_host: bad arguments or a key that is not live")
    return _result(out, P)


def refresh_raw(ctx: Optional[Context], store: Optional[KeyFrameStore], K, keys, kf_center, P, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, nlevels, scale_factors,
                out: dict) -> int:
    """the return code on raw arguments (None: a null pointer; out: the six output arrays by name, None allowed); ctx = None calls the host evaluator.  The refusal
    tests call this"""
    a = _inputs(keys, kf_center, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, scale_factors)
    p = [_p(x) for x in a]
    outs = [_p(out[k]) for k in ("best_obs", "best_desc", "normal", "min_dist", "max_dist", "status")]
    if ctx is None:
        return int(_host().ccmh_mappoint_refresh_eval_resident_host(None if store is None else store.handle, int(K), p[0], p[1], int(P), *p[2:8], int(nlevels), p[8], *outs))
    return int(_dev().ccm_mappoint_refresh_resident(ctx.handle, None if store is None else store.raw, int(K), p[0], p[1], int(P), *p[2:8], int(nlevels), p[8], *outs))


class Refresh:
    """cslam::MapPointRefresh: the constructor makes the one device call (host=True or a host-only store: the host evaluation)"""

    def __init__(self, store: KeyFrameStore, keys, kf_center, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, scale_factors, normal, min_dist, max_dist, host: bool = False):
        a = _inputs(keys, kf_center, obs_off, obs_kf, obs_feat, pos, ref_kf, ref_feat, scale_factors)
        self.P = int(a[2].size) - 1
        seed = [np.ascontiguousarray(np.asarray(x, np.float32).reshape(-1)) for x in (normal, min_dist, max_dist)]
        self._h = _host().ccmh_mappoint_refresh_create(store.handle, -1 if host else store.device, int(a[0].size), _p(a[0]), _p(a[1]), self.P, *[_p(x) for x in a[2:8]],
                                                       *[_p(x) for x in seed], int(a[8].size), _p(a[8]))
        if not self._h:
            raise CcmError("ccmh_mappoint_refresh_create failed (bad arguments, a key that is not live or a device error)")

    def result(self) -> dict:
        """the accessors: best, descriptor(p) (has_desc[p]: not nullptr), normal, min_dist, max_dist, status"""
        P = self.P
        out = _outputs(P, None, None, None, True)
        has = np.zeros(P, np.uint8)
        if _host().ccmh_mappoint_refresh_result(self._h, P, _p(out["best_obs"]), _p(out["best_desc"]), _p(has), _p(out["normal"]), _p(out["min_dist"]), _p(out["max_dist"]),
                                                _p(out["status"])) != 0:
            raise CcmError("ccmh_mappoint_refresh_result failed")
        out["has_desc"] = has
        return _result(out, P)

    def close(self):
        if self._h:
            _host().ccmh_mappoint_refresh_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------------------------------------
# generator (numpy only; nothing here touches the device)
# ---------------------------------------------------------------------------------------------------------------------------------------------
PROFILE_KEYFRAMES = 21
PROFILE_SIZES = {"1000x2": dict(n_points=1000, mean_obs=2, tail=0), "1000x6": dict(n_points=1000, mean_obs=6, tail=0), "5000x15": dict(n_points=5000, mean_obs=15, tail=200)}
K4 = (458.654, 457.296, 367.215, 248.375)


def profile_scene(n_points: int, mean_obs: float, tail: int, seed: int = 0, nlevels: int = 8) -> dict:
    """A refresh after a map stage: 21 keyframes on a line looking at n_points points at depths 2 .. 8 m.  A point's observation count is 2 + a geometric draw of
    mean mean_obs - 2 (mean_obs == 2: every point has exactly 2, as CreateNewMapPoints leaves them), capped at 64; with tail > 0 one point in a hundred has between
    100 and `tail` observations (a server's old points).  Observers are drawn from the keyframes in turn, so a long list meets a keyframe more than once; every
    observation gets a feature of its own whose descriptor is the point's with 8 % of the bits flipped.  The reference keyframe is the first observer.
    Returns the store's arrays per keyframe (add_scene installs them) and the flat call arguments."""
    rng = np.random.default_rng(seed)
    K = PROFILE_KEYFRAMES
    if mean_obs <= 2:
        n_obs = np.full(n_points, 2, np.int64)
    else:
        n_obs = np.minimum(2 + rng.geometric(1.0 / (mean_obs - 1), n_points) - 1, 64)
    if tail > 0:
        old = rng.random(n_points) < 0.01
        n_obs[old] = rng.integers(100, tail + 1, int(old.sum()))
    obs_off = np.concatenate([[0], np.cumsum(n_obs)]).astype(np.int32)
    M = int(obs_off[-1])
    start = rng.integers(0, K, n_points)
    obs_kf = np.concatenate([(start[p] + np.arange(n_obs[p])) % K for p in range(n_points)]).astype(np.int32)
    # a feature of its own for every observation: its index is its rank among the keyframe's observations
    order = np.argsort(obs_kf, kind="stable")
    count = np.bincount(obs_kf, minlength=K)
    first = np.concatenate([[0], np.cumsum(count)])
    obs_feat = np.empty(M, np.int32)
    obs_feat[order] = (np.arange(M) - first[obs_kf[order]]).astype(np.int32)
    base = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    pt_of = np.repeat(np.arange(n_points), n_obs)
    bits = np.unpackbits(base[pt_of], axis=1)
    desc = np.packbits(bits ^ (rng.random(bits.shape) < 0.08), axis=1)
    octave = np.minimum(rng.geometric(0.45, M) - 1, nlevels - 1).astype(np.uint8)
    kfs = []
    for k in range(K):
        sel = order[first[k]:first[k + 1]]
        n = int(sel.size)
        kfs.append(dict(desc=np.ascontiguousarray(desc[sel]), octave=octave[sel].copy(), xy=np.stack([rng.uniform(20, 732, n), rng.uniform(20, 460, n)], 1).astype(np.float32)))
    pos = np.stack([rng.uniform(-3, 3, n_points), rng.uniform(-2, 2, n_points), rng.uniform(2, 8, n_points)], 1).astype(np.float32)
    kf_center = np.stack([0.1 * np.arange(K) - 1.0, 0.01 * (np.arange(K) % 3), np.zeros(K)], 1).astype(np.float32)
    ref_kf = obs_kf[obs_off[:-1]].copy()
    ref_feat = obs_feat[obs_off[:-1]].copy()
    sf = (np.float32(1.2) ** np.arange(nlevels)).astype(np.float32)
    return dict(K=K, kfs=kfs, keys=np.arange(K, dtype=np.int64), kf_center=kf_center, obs_off=obs_off, obs_kf=obs_kf, obs_feat=obs_feat, pos=pos, ref_kf=ref_kf,
                ref_feat=ref_feat, scale_factors=sf, max_feat=int(count.max()),
                normal=np.zeros((n_points, 3), np.float32), min_dist=np.zeros(n_points, np.float32), max_dist=np.zeros(n_points, np.float32))


def add_scene(store: KeyFrameStore, scene: dict):
    """the keyframes of a profile_scene under its keys"""
    rec = fs.kf_record(np.asarray(K4, np.float32), fs.BOUNDS)
    for key, kf in zip(scene["keys"], scene["kfs"]):
        store.add([int(key)], rec, [0, kf["octave"].size], kf["xy"], kf["octave"], kf["desc"])


def call_args(scene: dict) -> tuple:
    """the positional arguments of refresh_resident / refresh_host after the store"""
    return tuple(scene[k] for k in ("keys", "kf_center", "obs_off", "obs_kf", "obs_feat", "pos", "ref_kf", "ref_feat", "scale_factors"))
