"""Sim3 correction of a closed loop's or merged map's keyframes and map points (LoopFinder.cpp:543-613, MapMerger.cpp:289-395, Optimizer.cpp:1279-1330).

correct_map is ccm_sim3_correct_map (include/ccm_hip.h): one packed copy in, a keyframe kernel and a point kernel, one copy out.  correct_map_host runs the
same lines compiled for the host (libccm_host.so).  MapCorrection is the host mirror cslam::Sim3MapCorrection: it takes the per-keyframe point lists and
per-point observation lists of the graph, assigns every point to the first keyframe of the walk that lists it, builds the ranks and makes the one call.
make_scene generates seeded maps (a chain of keyframes with covisibility, a drifted Sim3 with scale != 1) at the three sizes of SIZES; flatten_loop /
flatten_epilogue turn a scene into the flat arguments.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

import numpy as np

from . import synth
from ._lib import CcmError, Context, _arr, _p, check, host, lib

INT32_MAX = np.int32(2**31 - 1)
# keyframes of the corrected set, map points: a loop neighbourhood, one agent's map, the 4-agent map (about 6.4 observations per point)
SIZES = {"loop": (30, 3000), "agent": (500, 37500), "agents4": (2000, 150000)}

@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    h.ccmh_sim3corr_create_loop.restype = C.c_void_p
    h.ccmh_sim3corr_create_loop.argtypes = [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 9 + [C.c_int]
    h.ccmh_sim3corr_create_epilogue.restype = C.c_void_p
    h.ccmh_sim3corr_create_epilogue.argtypes = [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 9 + [C.c_int]
    h.ccmh_sim3corr_results.argtypes = [C.c_void_p] * 10
    h.ccmh_sim3corr_destroy.argtypes = [C.c_void_p]
    h.ccmh_sim3corr_destroy.restype = None
    h.ccmh_sim3_correct_map_host.argtypes = _FLAT_ARGTYPES
    return h


# ccm_sim3_correct_map after the context
_FLAT_ARGTYPES = [C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 8 + [C.c_int] + [C.c_void_p] * 6


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the flat call
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _flat_call(fn, first, f: dict):
    """f: the keys of flatten_loop / flatten_epilogue.  Returns a dict of the outputs; raises through `fn`'s return code."""
    Tiw = _arr(f.get("Tiw"), np.float32)
    n_kf = int(f["n_kf"])
    cen = _arr(f["kf_center"], np.float32); rank = _arr(f["kf_rank"], np.int32)
    n_obs_kf = cen.size // 3
    pos = _arr(f["pos"], np.float32)
    n_pt = int(f.get("n_pt", pos.size // 3))
    S_non = np.zeros(8 * max(n_kf, 1)) if Tiw is not None else _arr(f["S_non"], np.float64).copy()
    S_cor = np.zeros(8 * max(n_kf, 1)) if Tiw is not None else _arr(f["S_cor"], np.float64).copy()
    normal = _arr(f["normal"], np.float32).copy(); dmin = _arr(f["min_dist"], np.float32).copy(); dmax = _arr(f["max_dist"], np.float32).copy()
    sf = _arr(f["scale_factors"], np.float32)
    ins = [_arr(f[k], np.int32) for k in ("owner", "owner_rank", "obs_off", "obs_kf", "ref_kf", "ref_level")]
    pos_out = np.zeros(max(pos.size, 3), np.float32); T_new = np.zeros(12 * max(n_kf, 1), np.float32); c_new = np.zeros(3 * max(n_kf, 1), np.float32)
    rc = fn(*first, n_kf, _p(Tiw), int(f.get("cur", 0)), _p(_arr(f.get("Twc"), np.float32)), _p(_arr(f.get("Scw"), np.float64)), _p(S_non), _p(S_cor),
            int(f.get("n_obs_kf", n_obs_kf)), _p(cen), _p(rank), n_pt, _p(pos), *(_p(x) for x in ins), _p(sf), int(f.get("n_levels", sf.size)),
            _p(pos_out), _p(normal), _p(dmin), _p(dmax), _p(T_new), _p(c_new))
    out = dict(pos=pos_out[:3 * n_pt].reshape(-1, 3), normal=normal.reshape(-1, 3), min_dist=dmin, max_dist=dmax, Tiw=T_new.reshape(-1, 12),
               center=c_new.reshape(-1, 3), S_non=S_non.reshape(-1, 8), S_cor=S_cor.reshape(-1, 8))
    return rc, out


def correct_map(ctx: Context, flat: dict) -> dict:
    """ccm_sim3_correct_map on the arguments of flatten_loop / flatten_epilogue."""
    fn = lib().ccm_sim3_correct_map
    fn.argtypes = [C.c_void_p] + _FLAT_ARGTYPES
    rc, out = _flat_call(fn, (ctx.handle,), flat)
    check(rc, ctx.handle)
    return out


def correct_map_host(flat: dict) -> dict:
    """The same arguments through sim3_correct_math.h compiled for the host, on the calling thread (ccmh_sim3_correct_map_host)."""
    rc, out = _flat_call(_host().ccmh_sim3_correct_map_host, (), flat)
    if rc != 0:
        raise CcmError(f"ccmh_sim3_correct_map_host: bad arguments ({rc})")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the host mirror
# ---------------------------------------------------------------------------------------------------------------------------------------------
class MapCorrection:
    """cslam::Sim3MapCorrection.  device None: the host evaluator, asked for by name.  `scene`: the keys of make_scene."""

    def __init__(self, handle, n_kf, n_pt):
        if not handle:
            raise CcmError("ccmh_sim3corr_create: bad arguments or device error")
        self._h = C.c_void_p(handle)
        self.n_kf, self.n_pt = n_kf, n_pt

    @staticmethod
    def _points(sc):
        return [_arr(sc["pos"], np.float32), _arr(sc["normal"], np.float32), _arr(sc["min_dist"], np.float32), _arr(sc["max_dist"], np.float32),
                _arr(sc["obs_off"], np.int32), _arr(sc["obs_kf"], np.int32), _arr(sc["ref_kf"], np.int32), _arr(sc["ref_level"], np.int32)]

    @classmethod
    def loop(cls, sc: dict, device: Optional[int] = None):
        a = [_arr(sc["Tiw"], np.float32), _arr(sc["kf_center"], np.float32)]
        b = [_arr(sc["Twc"], np.float32), _arr(sc["Scw"], np.float64), _arr(sc["list_off"], np.int32), _arr(sc["list_pt"], np.int32), _arr(sc["list_skip"], np.uint8)]
        pts = cls._points(sc); sf = _arr(sc["scale_factors"], np.float32)
        n_kf = a[0].size // 12; n_pt = pts[2].size
        h = _host().ccmh_sim3corr_create_loop(-1 if device is None else int(device), n_kf, a[1].size // 3, _p(a[0]), _p(a[1]), int(sc["cur"]), *(_p(x) for x in b), n_pt,
                                              *(_p(x) for x in pts), _p(sf), int(sf.size))
        return cls(h, n_kf, n_pt)

    @classmethod
    def epilogue(cls, sc: dict, S_non, S_cor, pt_kf, device: Optional[int] = None):
        cen = _arr(sc["kf_center"], np.float32); S_non = _arr(S_non, np.float64); S_cor = _arr(S_cor, np.float64); pt_kf = _arr(pt_kf, np.int32)
        pts = cls._points(sc); sf = _arr(sc["scale_factors"], np.float32)
        n_kf = S_non.size // 8; n_pt = pts[2].size
        h = _host().ccmh_sim3corr_create_epilogue(-1 if device is None else int(device), n_kf, cen.size // 3, _p(cen), _p(S_non), _p(S_cor), _p(pt_kf), n_pt,
                                                  *(_p(x) for x in pts), _p(sf), int(sf.size))
        return cls(h, n_kf, n_pt)

    def results(self) -> dict:
        n, k = max(self.n_pt, 1), self.n_kf
        o = dict(pos=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), min_dist=np.zeros(n, np.float32), max_dist=np.zeros(n, np.float32),
                 tag=np.full(n, -1, np.int32), Tiw=np.zeros((k, 12), np.float32), center=np.zeros((k, 3), np.float32), S_non=np.zeros((k, 8)), S_cor=np.zeros((k, 8)))
        _host().ccmh_sim3corr_results(self._h, *(_p(o[x]) for x in ("pos", "normal", "min_dist", "max_dist", "tag", "Tiw", "center", "S_non", "S_cor")))
        for x in ("pos", "normal", "min_dist", "max_dist", "tag"):
            o[x] = o[x][:self.n_pt]
        return o

    def close(self):
        if self._h:
            _host().ccmh_sim3corr_destroy(self._h)
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
    """Rodrigues, f64; w: (..., 3)"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1] = -w[..., 2]; K[..., 0, 2] = w[..., 1]; K[..., 1, 0] = w[..., 2]; K[..., 1, 2] = -w[..., 0]; K[..., 2, 0] = -w[..., 1]; K[..., 2, 1] = w[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(th > 1e-12, np.sin(th) / th, 1.0); b = np.where(th > 1e-12, (1 - np.cos(th)) / (th * th), 0.5)
    return np.eye(3) + a * K + b * (K @ K)


def _quat(R):
    """unit quaternion x y z w of a rotation matrix (f64), w >= 0"""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    q = np.array([np.copysign(x, R[2, 1] - R[1, 2]), np.copysign(y, R[0, 2] - R[2, 0]), np.copysign(z, R[1, 0] - R[0, 1]), w])
    return q / np.linalg.norm(q)


def camera_center(T):
    """Ow of KeyFrame::SetPose for poses (n, 12) f32: -(Rcw' tcw), f32 products added left to right."""
    T = np.asarray(T, np.float32).reshape(-1, 12)
    O = np.zeros((T.shape[0], 3), np.float32)
    for r in range(3):
        t = T[:, r] * T[:, 3]
        t = t + T[:, 4 + r] * T[:, 7]
        t = t + T[:, 8 + r] * T[:, 11]
        O[:, r] = (t.astype(np.float64) * -1.0 + 0.0).astype(np.float32)
    return O


def make_scene(seed: int = 0, n_kf: int = 30, n_pt: int = 3000, n_out: Optional[int] = None, mean_obs: float = 6.4, window: int = 40, null_frac: float = 0.05,
               dup_frac: float = 0.01, bad_frac: float = 0.02, tagged_frac: float = 0.02, no_obs_frac: float = 0.003, stale_frac: float = 0.02, scale: float = 1.07) -> dict:
    """A chain of n_out + n_kf keyframes; the last n_kf chain positions are the corrected set (indices 0 .. n_kf - 1 in a random walk order), the others the
    observers outside it (indices n_kf ..).  Points sit along the chain and are seen by 2 .. 30 keyframes of a covisibility window, in random list order; the
    reference keyframe is the first of the list.  Keyframe i of the set lists the points that see it, plus null entries, repeated entries and entries of bad or
    already-tagged points (list_skip); a fraction `stale_frac` of the observations has a null entry in the keyframe's list instead.  Scw is the current keyframe's pose drifted by a small rotation, a translation and `scale`."""
    rng = np.random.default_rng(seed)
    if n_out is None:
        n_out = max(0, min(n_kf // 3, 200))
    n_all = n_kf + n_out
    # chain: a slowly turning path, one keyframe every 0.3 m
    s = np.arange(n_all) * 0.3
    centres = np.stack([8 * np.sin(s / 8), 0.3 * np.sin(s / 3), 8 * (1 - np.cos(s / 8)) + 0.2 * s], 1) + rng.normal(0, 0.03, (n_all, 3))
    Rcw = _rot(np.stack([rng.normal(0, 0.05, n_all), s / 8 + rng.normal(0, 0.05, n_all), rng.normal(0, 0.05, n_all)], 1))
    tcw = -(Rcw @ centres[:, :, None])[:, :, 0]
    # chain position -> keyframe index
    kf_of_chain = np.concatenate([n_kf + rng.permutation(n_out), rng.permutation(n_kf)]).astype(np.int32)
    T = np.zeros((n_all, 12), np.float32)
    T[kf_of_chain] = np.concatenate([Rcw, tcw[:, :, None]], 2).reshape(n_all, 12).astype(np.float32)
    kf_center = camera_center(T)
    cur = int(kf_of_chain[-1])
    Rc = T[cur].reshape(3, 4)[:, :3]
    Twc = np.concatenate([Rc.T, kf_center[cur][:, None]], 1).reshape(12).astype(np.float32)
    dR = _rot(rng.normal(0, 0.04, 3))
    Rn = dR @ T[cur].reshape(3, 4)[:, :3].astype(np.float64)
    tn = scale * (dR @ T[cur].reshape(3, 4)[:, 3].astype(np.float64)) + rng.normal(0, 0.3, 3)
    Scw = np.concatenate([_quat(Rn), tn, [scale]])
    # points and their observers
    W = min(window, n_all)
    base_chain = rng.integers(0, n_all, n_pt) if n_out == 0 else np.minimum(n_all - 1, n_out // 2 + rng.integers(0, n_all - n_out // 2, n_pt))
    pos = (centres[base_chain] + rng.normal(0, 1.0, (n_pt, 3)) + (Rcw[base_chain].transpose(0, 2, 1) @ np.array([0, 0, 4.0]))).astype(np.float32)
    cnt = np.minimum(np.minimum(30, W), np.maximum(min(2, W), 2 + rng.geometric(1.0 / max(mean_obs - 1.0, 1.0), n_pt) - 1)).astype(np.int64)
    cnt[rng.random(n_pt) < no_obs_frac] = 0
    lo = np.clip(base_chain - W // 2, 0, n_all - W)
    order = np.argsort(rng.random((n_pt, W)), axis=1)
    keep = np.arange(W)[None, :] < cnt[:, None]
    obs_kf = kf_of_chain[(lo[:, None] + order)[keep]].astype(np.int32)
    obs_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    obs_pt = np.repeat(np.arange(n_pt), cnt)
    ref_kf = np.where(cnt > 0, obs_kf[np.minimum(obs_off[:-1], max(obs_kf.size - 1, 0))] if obs_kf.size else 0, kf_of_chain[base_chain]).astype(np.int32)
    ref_level = rng.integers(0, 8, n_pt).astype(np.int32)
    normal = rng.normal(0, 1, (n_pt, 3)).astype(np.float32)
    max_dist = rng.uniform(2, 20, n_pt).astype(np.float32); min_dist = (max_dist * np.float32(0.3)).astype(np.float32)
    # the keyframes' lists
    in_set = obs_kf < n_kf
    lk, lp = obs_kf[in_set].astype(np.int64), obs_pt[in_set].astype(np.int64)
    n_e = lk.size
    lp[rng.random(n_e) < stale_frac] = -1   # an observation whose keyframe no longer lists the point: that observer can be walked before the point's owner
    extra_k, extra_p = [], []
    n_null, n_dup = int(null_frac * n_e), int(dup_frac * n_e)
    extra_k.append(rng.integers(0, n_kf, n_null)); extra_p.append(np.full(n_null, -1))
    if n_e and n_dup:
        d = rng.integers(0, n_e, n_dup)
        extra_k.append(lk[d]); extra_p.append(lp[d])
    lonely = np.nonzero(cnt == 0)[0]
    extra_k.append(rng.integers(0, n_kf, lonely.size)); extra_p.append(lonely)
    lk = np.concatenate([lk] + extra_k); lp = np.concatenate([lp] + extra_p)
    sh = rng.permutation(lk.size)
    lk, lp = lk[sh], lp[sh]
    so = np.argsort(lk, kind="stable")
    lk, lp = lk[so], lp[so]
    list_off = np.concatenate([[0], np.cumsum(np.bincount(lk, minlength=n_kf))]).astype(np.int32)
    bad = rng.random(n_pt) < bad_frac; tagged = rng.random(n_pt) < tagged_frac
    list_skip = np.where(lp >= 0, (bad | tagged)[np.maximum(lp, 0)], False).astype(np.uint8)
    sf = synth.scale_tables()[0].astype(np.float32)
    return dict(n_kf=n_kf, n_obs_kf=n_all, Tiw=T[:n_kf].copy(), T_all=T, kf_center=kf_center, cur=cur, Twc=Twc, Scw=Scw, pos=pos, normal=normal, min_dist=min_dist,
                max_dist=max_dist, obs_off=obs_off, obs_kf=obs_kf, ref_kf=ref_kf, ref_level=ref_level, list_off=list_off, list_pt=lp.astype(np.int32),
                list_skip=list_skip, scale_factors=sf)


def owners(sc: dict) -> np.ndarray:
    """Per point the first keyframe of the walk that lists it through an entry that is not skipped, -1 if none."""
    lp = np.asarray(sc["list_pt"]); lk = np.repeat(np.arange(sc["n_kf"]), np.diff(sc["list_off"]))
    ok = (lp >= 0) & (np.asarray(sc["list_skip"]) == 0)
    own = np.full(np.asarray(sc["min_dist"]).size, np.iinfo(np.int32).max, np.int64)
    np.minimum.at(own, lp[ok], lk[ok])
    own[own == np.iinfo(np.int32).max] = -1
    return own.astype(np.int32)


def _compact(sc: dict, own: np.ndarray, owner_rank) -> dict:
    sel = np.nonzero(own >= 0)[0]
    off = np.asarray(sc["obs_off"], np.int64)
    cnt = (off[1:] - off[:-1])[sel]
    idx = np.repeat(off[:-1][sel], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    n_obs_kf = np.asarray(sc["kf_center"]).size // 3
    rank = np.full(n_obs_kf, INT32_MAX, np.int32); rank[:sc["n_kf"]] = np.arange(sc["n_kf"])
    f = dict(n_kf=sc["n_kf"], kf_center=sc["kf_center"], kf_rank=rank, sel=sel, pos=np.asarray(sc["pos"], np.float32).reshape(-1, 3)[sel], owner=own[sel],
             owner_rank=(rank[own[sel]] if owner_rank is None else np.full(sel.size, owner_rank, np.int32)),
             obs_off=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), obs_kf=np.asarray(sc["obs_kf"], np.int32)[idx.astype(np.int64)],
             ref_kf=np.asarray(sc["ref_kf"])[sel], ref_level=np.asarray(sc["ref_level"])[sel], scale_factors=sc["scale_factors"],
             normal=np.asarray(sc["normal"], np.float32).reshape(-1, 3)[sel], min_dist=np.asarray(sc["min_dist"])[sel], max_dist=np.asarray(sc["max_dist"])[sel])
    return f


def flatten_loop(sc: dict) -> dict:
    """The arguments of correct_map / correct_map_host for the loop / merge form of a scene (what cslam::Sim3MapCorrection builds); `sel`: the points sent."""
    f = _compact(sc, owners(sc), None)
    f.update(Tiw=sc["Tiw"], cur=sc["cur"], Twc=sc["Twc"], Scw=sc["Scw"])
    return f


def flatten_epilogue(sc: dict, S_non, S_cor, pt_kf) -> dict:
    """The arguments for the essential-graph epilogue form: every point with pt_kf >= 0 moves with that keyframe's pair, every keyframe of the set shows its new centre."""
    f = _compact(sc, np.asarray(pt_kf, np.int32), INT32_MAX)
    f.update(Tiw=None, S_non=S_non, S_cor=S_cor)
    return f
