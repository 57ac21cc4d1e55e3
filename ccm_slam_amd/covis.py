"""The covisibility graph of a corrected map: KeyFrame::UpdateConnections (KeyFrame.cpp:629-711) over a set of keyframes in walk order, with the AddConnection /
UpdateBestCovisibles calls (:392-426) they make on each other (LoopFinder.cpp:612 / :655, MapMerger.cpp:392 / :487, Map.cpp:614).

update is ccm_covis_update (include/ccm_hip.h): one packed copy in, seven launches, one copy out.  update_host runs the same rules (csrc/covis_math.h) compiled
for the host (libccm_host.so).  CovisibilityBatch is the host mirror cslam::CovisibilityBatch: the one call, the AddConnection calls for keyframes outside the set
and the GetBestCovisibilityKeyFrames / GetCovisiblesByWeight views.  make_scene generates seeded maps (a chain of keyframes with a covisibility window; stale,
repeated, null and bad list entries; a shuffled order_key) at the sizes of sim3_correct.SIZES; reorder gives the same map under another walk order.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

import numpy as np

from ._lib import CcmError, Context, _arr, _p, check, hooks, host, lib
from .sim3_correct import SIZES  # noqa: F401  (the three sizes the profile runs at)

EMPTY, FALLBACK, CHANGED = 1, 2, 4
TH = 15   # KeyFrame.cpp:673
_OUT = ("row_off", "col", "count", "fw_off", "fw_col", "fw_w", "ord_off", "ord_kf", "ord_w", "flags")
# ccm_covis_update after the context
_FLAT_ARGTYPES = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int, C.c_int] + [C.c_void_p] * 11

@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    h.ccmh_covis_create.restype = C.c_void_p
    h.ccmh_covis_create.argtypes = [C.c_int] * 3 + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int]
    h.ccmh_covis_sizes.argtypes = [C.c_void_p] * 2
    h.ccmh_covis_results.argtypes = [C.c_void_p] * 12
    h.ccmh_covis_best.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    h.ccmh_covis_by_weight.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    h.ccmh_covis_destroy.argtypes = [C.c_void_p]
    h.ccmh_covis_destroy.restype = None
    h.ccmh_covis_update_host.argtypes = _FLAT_ARGTYPES
    return h


_DEVICE = {}


def _device(small_window: bool):
    """ccm_covis_update, or the test hook with a histogram window of 64 keyframe indices; argument types set once"""
    if small_window not in _DEVICE:
        fn = hooks().ccm_debug_covis_update_small if small_window else lib().ccm_covis_update
        fn.argtypes = [C.c_void_p] + _FLAT_ARGTYPES
        _DEVICE[small_window] = fn
    return _DEVICE[small_window]


def _inputs(sc: dict):
    key = _arr(sc["order_key"], np.int32); loff = _arr(sc["list_off"], np.int32); lpt = _arr(sc["list_pt"], np.int32); skip = _arr(sc["list_skip"], np.uint8)
    ooff = _arr(sc["obs_off"], np.int32); okf = _arr(sc["obs_kf"], np.int32)
    n_kf = int(sc.get("n_kf", loff.size - 1)); n_all = int(sc.get("n_all", key.size)); n_pt = int(sc.get("n_pt", ooff.size - 1))
    return n_kf, n_all, n_pt, key, loff, lpt, skip, ooff, okf


def call(fn, first, sc: dict, th: int = TH, cap: int = 4096):
    """One call of `fn` (ccm_covis_update or a function with its arguments) on the keys of make_scene with capacity `cap`: (return code, outputs, needed[3])."""
    n_kf, n_all, n_pt, key, loff, lpt, skip, ooff, okf = _inputs(sc)
    k = max(n_kf, 1)
    o = {x: np.zeros(k + 1 if x.endswith("_off") else k if x == "flags" else max(cap, 1), np.int32) for x in _OUT}
    needed = np.zeros(3, np.int32)
    rc = fn(*first, n_kf, n_all, _p(key), _p(loff), _p(lpt), _p(skip), n_pt, _p(ooff), _p(okf), int(th), int(cap), *(_p(o[x]) for x in _OUT), _p(needed))
    return rc, o, needed


def _complete(fn, first, sc, th, cap, on_error):
    n_kf = _inputs(sc)[0]
    cap = max(4096, 96 * n_kf) if cap is None else int(cap)
    for attempt in range(4):
        rc, o, needed = call(fn, first, sc, th, cap)
        if rc != 0:
            on_error(rc)
        if needed.max() <= cap:
            o["col"], o["count"] = o["col"][:needed[0]], o["count"][:needed[0]]
            o["fw_col"], o["fw_w"] = o["fw_col"][:needed[1]], o["fw_w"][:needed[1]]
            o["ord_kf"], o["ord_w"] = o["ord_kf"][:needed[2]], o["ord_w"][:needed[2]]
            o["calls"] = attempt + 1
            return o
        cap = 2 * int(needed.max())   # the final rows are at most twice the count rows
    raise CcmError("ccm_covis_update: the capacity asked for keeps growing")


def update(ctx: Context, sc: dict, th: int = TH, cap: Optional[int] = None, small_window: bool = False) -> dict:
    """ccm_covis_update on the keys of make_scene; calls again with the capacity asked for when `cap` was too small.  small_window: the test hook with a
    histogram window of 64 keyframe indices."""
    return _complete(_device(small_window), (ctx.handle,), sc, th, cap, lambda rc: check(rc, ctx.handle))


def update_host(sc: dict, th: int = TH, cap: Optional[int] = None) -> dict:
    """The same arguments through covis_math.h compiled for the host, on the calling thread (ccmh_covis_update_host)."""
    def bad(rc):
        raise CcmError(f"ccmh_covis_update_host: bad arguments ({rc})")
    return _complete(_host().ccmh_covis_update_host, (), sc, th, cap, bad)


class CovisibilityBatch:
    """cslam::CovisibilityBatch.  device None: the host evaluator, asked for by name.  `sc`: the keys of make_scene."""

    def __init__(self, sc: dict, th: int = TH, device: Optional[int] = None):
        n_kf, n_all, n_pt, key, loff, lpt, skip, ooff, okf = _inputs(sc)
        h = _host().ccmh_covis_create(-1 if device is None else int(device), n_kf, n_all, _p(key), _p(loff), _p(lpt), _p(skip), n_pt, _p(ooff), _p(okf), int(th))
        if not h:
            raise CcmError("ccmh_covis_create: bad arguments or device error")
        self._h = C.c_void_p(h)
        self.n_kf = n_kf

    def results(self) -> dict:
        s = np.zeros(5, np.int64)
        _host().ccmh_covis_sizes(self._h, _p(s))
        k = self.n_kf
        size = dict(flags=k, row_off=k + 1, col=s[1], count=s[1], fw_off=k + 1, fw_col=s[2], fw_w=s[2], ord_off=k + 1, ord_kf=s[3], ord_w=s[3], outside=3 * s[4])
        names = ("flags", "row_off", "col", "count", "fw_off", "fw_col", "fw_w", "ord_off", "ord_kf", "ord_w", "outside")
        o = {x: np.zeros(int(size[x]), np.int32) for x in names}
        _host().ccmh_covis_results(self._h, *(_p(o[x]) if o[x].size else None for x in names))
        o["outside"] = o["outside"].reshape(-1, 3)   # target, source, weight
        return o

    def _view(self, fn, i, arg):
        n = fn(self._h, int(i), int(arg), None, 0)
        if n < 0:
            raise CcmError("CovisibilityBatch: keyframe outside the set")
        out = np.zeros(max(n, 1), np.int32)
        fn(self._h, int(i), int(arg), _p(out), n)
        return out[:n]

    def best_covisibles(self, i: int, n: int) -> np.ndarray:
        """GetBestCovisibilityKeyFrames(n) of keyframe i"""
        return self._view(_host().ccmh_covis_best, i, n)

    def covisibles_by_weight(self, i: int, w: int) -> np.ndarray:
        """GetCovisiblesByWeight(w) of keyframe i (empty when every weight is >= w, as in the reference)"""
        return self._view(_host().ccmh_covis_by_weight, i, w)

    def close(self):
        if self._h:
            _host().ccmh_covis_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def make_scene(seed: int = 0, n_kf: int = 30, n_pt: int = 3000, n_out: Optional[int] = None, mean_obs: float = 6.4, window: int = 40, max_obs: int = 30,
               null_frac: float = 0.05, dup_frac: float = 0.01, bad_frac: float = 0.02, stale_frac: float = 0.02) -> dict:
    """A chain of n_out + n_kf keyframes; the last n_kf chain positions are the set (indices 0 .. n_kf - 1 in a random walk order), the others the observers
    outside it (indices n_kf ..).  A point is seen by 2 .. max_obs keyframes of a window of `window` chain positions.  Keyframe i of the set lists the points that
    see it, except a fraction `stale_frac` (the observation stays, the entry is null: C_i[j] and C_j[i] then differ), plus null entries and repeated entries;
    list_skip marks the entries of bad points.  order_key is a shuffled set of distinct values, some negative."""
    rng = np.random.default_rng(seed)
    if n_out is None:
        n_out = max(0, min(n_kf // 3, 200))
    n_all = n_kf + n_out
    kf_of_chain = np.concatenate([n_kf + rng.permutation(n_out), rng.permutation(n_kf)]).astype(np.int32)
    W = min(window, n_all)
    base_chain = rng.integers(0, n_all, n_pt)
    cnt = np.minimum(min(max_obs, W), np.maximum(min(2, W), 1 + rng.geometric(1.0 / max(mean_obs - 1.0, 1.0), n_pt))).astype(np.int64)
    lo = np.clip(base_chain - W // 2, 0, n_all - W)
    order = np.argsort(rng.random((n_pt, W)), axis=1)
    keep = np.arange(W)[None, :] < cnt[:, None]
    obs_kf = kf_of_chain[(lo[:, None] + order)[keep]].astype(np.int32)
    obs_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    obs_pt = np.repeat(np.arange(n_pt), cnt)
    in_set = obs_kf < n_kf
    lk, lp = obs_kf[in_set].astype(np.int64), obs_pt[in_set].astype(np.int64)
    n_e = lk.size
    lp[rng.random(n_e) < stale_frac] = -1
    n_null, n_dup = int(null_frac * n_e), int(dup_frac * n_e)
    extra_k, extra_p = [rng.integers(0, n_kf, n_null)], [np.full(n_null, -1)]
    if n_e and n_dup:
        d = rng.integers(0, n_e, n_dup)
        extra_k.append(lk[d]); extra_p.append(lp[d])
    lk = np.concatenate([lk] + extra_k); lp = np.concatenate([lp] + extra_p)
    sh = rng.permutation(lk.size)
    lk, lp = lk[sh], lp[sh]
    so = np.argsort(lk, kind="stable")
    lk, lp = lk[so], lp[so]
    list_off = np.concatenate([[0], np.cumsum(np.bincount(lk, minlength=n_kf))]).astype(np.int32)
    bad = rng.random(n_pt) < bad_frac
    list_skip = np.where(lp >= 0, bad[np.maximum(lp, 0)], False).astype(np.uint8)
    order_key = (rng.permutation(n_all).astype(np.int64) * 7 - 3 * n_all).astype(np.int32)
    return dict(n_kf=n_kf, n_all=n_all, n_pt=n_pt, order_key=order_key, list_off=list_off, list_pt=lp.astype(np.int32), list_skip=list_skip, obs_off=obs_off,
                obs_kf=obs_kf)


def reorder(sc: dict, walk) -> dict:
    """The same map with the set walked in another order: walk[r] = the keyframe of `sc` that is walked r-th.  Keyframe indices are renamed accordingly
    (new index r = old index walk[r]; the outside keyframes keep theirs); order_key follows the keyframes."""
    n_kf, n_all = int(sc["n_kf"]), int(sc["n_all"])
    walk = np.asarray(walk, np.int64)
    assert sorted(walk.tolist()) == list(range(n_kf))
    old_of_new = np.concatenate([walk, np.arange(n_kf, n_all)])
    new_of_old = np.empty(n_all, np.int64); new_of_old[old_of_new] = np.arange(n_all)
    loff = np.asarray(sc["list_off"], np.int64)
    seg = [np.arange(loff[k], loff[k + 1]) for k in walk]
    idx = np.concatenate(seg) if seg else np.zeros(0, np.int64)
    out = dict(sc)
    out.update(order_key=np.asarray(sc["order_key"], np.int32)[old_of_new], list_off=np.concatenate([[0], np.cumsum([s.size for s in seg])]).astype(np.int32),
               list_pt=np.asarray(sc["list_pt"], np.int32)[idx], list_skip=np.asarray(sc["list_skip"], np.uint8)[idx],
               obs_kf=new_of_old[np.asarray(sc["obs_kf"], np.int64)].astype(np.int32), old_of_new=old_of_new.astype(np.int32))
    return out
