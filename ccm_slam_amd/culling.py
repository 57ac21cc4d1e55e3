"""The server's keyframe culling walk: LocalMapping::KeyFrameCullingV3 (Mapping.cpp:804-862) over the covisible keyframes of the picked keyframe in walk order, with
what culling one of them does to the points it sees (KeyFrame::SetBadFlag, KeyFrame.cpp:990-997; MapPoint::EraseObservation, MapPoint.cpp:442-509).

walk is ccm_kfcull_walk (include/ccm_hip.h): one packed copy in, two launches, one copy out.  walk_host runs the same rules (csrc/kfcull_math.h) compiled for the
host (libccm_host.so), walk_mapcopy_model the same walk on std::map observations copied per checked slot (a cost model of the reference's containers).
KeyFrameCullingBatch is the host mirror cslam::KeyFrameCullingBatch.  make_scene generates seeded neighbourhoods: a chain of keyframes with a covisibility window, a
share of well-observed points seen at one scale by every observer (the redundant ones), stale, repeated and null slots, bad observers and bad points, SKIP and
NOT_ERASE candidates and a pt_nobs that differs from the list's length; reorder gives the same scene under another walk order.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

import numpy as np

from ._lib import CcmError, Context, _arr, _p, check, host, lib

SKIP, NOT_ERASE = 1, 2
KEPT, CULLED, SKIPPED, REDUNDANT_NOT_ERASED = 0, 1, 2, 3
TH_OBS = 3        # Mapping.cpp:815
THRES = 0.98      # Mapping.RedThres of the reference's configuration
N_LEVELS = 8
# (n_cand, slots per candidate): a usual covisibility neighbourhood and a wide one, the sizes scripts/kfcull_profile.py runs at
SIZES = {"local": (30, 1000), "wide": (80, 1500)}
_OUT = (("verdict", np.uint8, "c"), ("n_mps", np.int32, "c"), ("n_red", np.int32, "c"), ("pt_gone", np.uint8, "p"), ("pt_nobs_out", np.int32, "p"))
# ccm_kfcull_walk after the context, up to n_levels
_IN_ARGTYPES = [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_double, C.c_int]
_FLAT_ARGTYPES = _IN_ARGTYPES + [C.c_void_p] * 6

@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    h.ccmh_kfcull_create.restype = C.c_void_p
    h.ccmh_kfcull_create.argtypes = [C.c_int] + _IN_ARGTYPES
    h.ccmh_kfcull_results.argtypes = [C.c_void_p] * 7
    h.ccmh_kfcull_culled.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    h.ccmh_kfcull_points_gone.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    h.ccmh_kfcull_destroy.argtypes = [C.c_void_p]
    h.ccmh_kfcull_destroy.restype = None
    h.ccmh_kfcull_walk_host.argtypes = _FLAT_ARGTYPES
    h.ccmh_kfcull_walk_mapcopy_model.argtypes = _IN_ARGTYPES + [C.c_void_p]
    return h


_DEVICE = None


def _device():
    """ccm_kfcull_walk; argument types set once"""
    global _DEVICE
    if _DEVICE is None:
        fn = lib().ccm_kfcull_walk
        fn.argtypes = [C.c_void_p] + _FLAT_ARGTYPES
        _DEVICE = fn
    return _DEVICE


def _inputs(sc: dict, th_obs, thres, n_levels):
    """the arguments of ccm_kfcull_walk after the context, up to n_levels, and the arrays that back them"""
    fl = _arr(sc["cand_flags"], np.uint8); loff = _arr(sc["list_off"], np.int32); lpt = _arr(sc["list_pt"], np.int32); llev = _arr(sc["list_level"], np.uint8)
    nobs = _arr(sc["pt_nobs"], np.int32); bad = _arr(sc["pt_bad"], np.uint8); ooff = _arr(sc["obs_off"], np.int32); okf = _arr(sc["obs_kf"], np.int32)
    olev = _arr(sc["obs_level"], np.uint8); obad = _arr(sc["obs_bad"], np.uint8)
    n_cand = int(sc.get("n_cand", loff.size - 1 if loff is not None else 0)); n_all = int(sc["n_all"])
    n_pt = int(sc.get("n_pt", ooff.size - 1 if ooff is not None else 0))
    keep = (fl, loff, lpt, llev, nobs, bad, ooff, okf, olev, obad)
    n_levels = int(sc.get("n_levels", N_LEVELS) if n_levels is None else n_levels)
    args = (n_cand, n_all, _p(fl), _p(loff), _p(lpt), _p(llev), n_pt, _p(nobs), _p(bad), _p(ooff), _p(okf), _p(olev), _p(obad), int(th_obs), float(thres), n_levels)
    return n_cand, n_pt, args, keep


def call(fn, first, sc: dict, thres: float = THRES, th_obs: int = TH_OBS, n_levels: Optional[int] = None, null_out: Optional[str] = None):
    """One call of `fn` (ccm_kfcull_walk or a function with its arguments) on the keys of make_scene: (return code, outputs).  null_out names an output passed as
    NULL."""
    n_cand, n_pt, args, keep = _inputs(sc, th_obs, thres, n_levels)
    o = {x: np.zeros(max(n_cand if w == "c" else n_pt, 1), dt) for x, dt, w in _OUT}
    n_reeval = np.full(1, -1, np.int32)
    outs = [None if x == null_out else _p(o[x]) for x, _, _ in _OUT] + [None if null_out == "n_reeval" else _p(n_reeval)]
    rc = fn(*first, *args, *outs)
    o = {x: o[x][:max(n_cand, 0) if w == "c" else max(n_pt, 0)] for x, _, w in _OUT}
    o["n_reeval"] = int(n_reeval[0])
    return rc, o


def walk(ctx: Context, sc: dict, thres: float = THRES, th_obs: int = TH_OBS, n_levels: Optional[int] = None) -> dict:
    """ccm_kfcull_walk on the keys of make_scene: verdict, n_mps, n_red per candidate, pt_gone, pt_nobs_out per point, n_reeval."""
    rc, o = call(_device(), (ctx.handle,), sc, thres, th_obs, n_levels)
    check(rc, ctx.handle)
    return o


def walk_host(sc: dict, thres: float = THRES, th_obs: int = TH_OBS, n_levels: Optional[int] = None) -> dict:
    """The same arguments through kfcull_math.h compiled for the host, on the calling thread (ccmh_kfcull_walk_host)."""
    rc, o = call(_host().ccmh_kfcull_walk_host, (), sc, thres, th_obs, n_levels)
    if rc != 0:
        raise CcmError(f"ccmh_kfcull_walk_host: bad arguments ({rc})")
    return o


def walk_mapcopy_model(sc: dict, thres: float = THRES, th_obs: int = TH_OBS, n_levels: Optional[int] = None) -> np.ndarray:
    """The verdicts of the same walk made on std::map observations that are copied for every checked slot, as the reference's containers make it: a cost model."""
    n_cand, _, args, keep = _inputs(sc, th_obs, thres, n_levels)
    verdict = np.zeros(max(n_cand, 1), np.uint8)
    if _host().ccmh_kfcull_walk_mapcopy_model(*args, _p(verdict)) != 0:
        raise CcmError("ccmh_kfcull_walk_mapcopy_model: bad arguments")
    return verdict[:n_cand]


class KeyFrameCullingBatch:
    """cslam::KeyFrameCullingBatch.  device None: the host evaluator, asked for by name.  `sc`: the keys of make_scene."""

    def __init__(self, sc: dict, thres: float = THRES, device: Optional[int] = None, th_obs: int = TH_OBS, n_levels: Optional[int] = None):
        self.n_cand, self.n_pt, args, keep = _inputs(sc, th_obs, thres, n_levels)
        h = _host().ccmh_kfcull_create(-1 if device is None else int(device), *args)
        if not h:
            raise CcmError("ccmh_kfcull_create: bad arguments or device error")
        self._h = C.c_void_p(h)

    def results(self) -> dict:
        o = {x: np.zeros(max(self.n_cand if w == "c" else self.n_pt, 1), dt) for x, dt, w in _OUT}
        n_reeval = np.zeros(1, np.int32)
        _host().ccmh_kfcull_results(self._h, *(_p(o[x]) for x, _, _ in _OUT), _p(n_reeval))
        o = {x: o[x][:self.n_cand if w == "c" else self.n_pt] for x, _, w in _OUT}
        o["n_reeval"] = int(n_reeval[0])
        return o

    def _view(self, fn):
        n = fn(self._h, None, 0)
        out = np.zeros(max(n, 1), np.int32)
        fn(self._h, _p(out), n)
        return out[:n]

    def culled(self) -> np.ndarray:
        """the candidates the caller calls SetBadFlag on (verdicts 1 and 3), in walk order"""
        return self._view(_host().ccmh_kfcull_culled)

    def points_gone(self) -> np.ndarray:
        """the points the walk turned bad"""
        return self._view(_host().ccmh_kfcull_points_gone)

    def close(self):
        if self._h:
            _host().ccmh_kfcull_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def make_scene(seed: int = 0, n_cand: int = 30, n_out: Optional[int] = None, n_pt: int = 3000, fine_frac: float = 0.93, fine_obs=(4, 7), mean_obs: float = 4.0,
               max_obs: int = 30, window: int = 12, stale_frac: float = 0.02, dup_frac: float = 0.01, null_frac: float = 0.05, bad_kf_frac: float = 0.1,
               bad_pt_frac: float = 0.02, skip_frac: float = 0.07, not_erase_frac: float = 0.07, nobs_off_frac: float = 0.05, n_levels: int = N_LEVELS) -> dict:
    """A chain of n_out + n_cand keyframes; a random subset of chain positions are the candidates (indices 0 .. n_cand - 1 in a random walk order), the others the
    observers outside the walk (indices n_cand ..), a share bad_kf_frac of them bad.  A share fine_frac of the points is well observed at a fine scale: fine_obs[0] ..
    fine_obs[1] keyframes of a window of `window` chain positions see it, all at one octave, so every observer finds the others redundant until erasures bring
    Observations() down to th_obs.  The other points have 2 .. max_obs observers (1 + geometric with mean mean_obs) at random octaves.  Candidate k has a slot for
    every point that lists it, plus stale slots (points that do not list it), repeated slots and null slots.  pt_nobs is the list's length except for a share
    nobs_off_frac of the points (-1, +1, +2); a share bad_pt_frac is bad, and so is a point without a non-bad observer (a live point has a reference keyframe)."""
    rng = np.random.default_rng(seed)
    if n_out is None:
        n_out = max(2, n_cand // 3)
    n_all = n_cand + n_out
    kf_of_chain = np.empty(n_all, np.int64)
    chain = rng.permutation(n_all)
    kf_of_chain[chain[:n_cand]] = rng.permutation(n_cand)
    kf_of_chain[chain[n_cand:]] = n_cand + rng.permutation(n_out)
    W = min(window, n_all)
    fine = rng.random(n_pt) < fine_frac
    cnt = np.where(fine, rng.integers(fine_obs[0], fine_obs[1] + 1, n_pt), 1 + rng.geometric(1.0 / max(mean_obs - 1.0, 1.0), n_pt))
    cnt = np.minimum(min(max_obs, W), np.maximum(min(2, W), cnt)).astype(np.int64)
    lo = np.clip(rng.integers(0, n_all, n_pt) - W // 2, 0, n_all - W)
    order = np.argsort(rng.random((n_pt, W)), axis=1)
    keep = np.arange(W)[None, :] < cnt[:, None]
    obs_kf = kf_of_chain[(lo[:, None] + order)[keep]].astype(np.int32)
    obs_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    obs_pt = np.repeat(np.arange(n_pt), cnt)
    base_level = rng.integers(0, n_levels, n_pt)
    obs_level = np.where(fine[obs_pt], base_level[obs_pt], rng.integers(0, n_levels, obs_kf.size)).astype(np.uint8)
    kf_bad = np.zeros(n_all, bool)
    kf_bad[n_cand:] = rng.random(n_out) < bad_kf_frac
    obs_bad = kf_bad[obs_kf].astype(np.uint8)
    live = np.zeros(n_pt, np.int64)
    np.add.at(live, obs_pt, 1 - obs_bad.astype(np.int64))
    pt_bad = ((rng.random(n_pt) < bad_pt_frac) | (live == 0)).astype(np.uint8)
    pt_nobs = cnt.copy()
    off = rng.random(n_pt) < nobs_off_frac
    pt_nobs[off] += rng.choice([-1, 1, 2], int(off.sum()))
    # the slots: one per observation by a candidate, then stale, repeated and null ones
    in_set = obs_kf < n_cand
    lk, lp, ll = obs_kf[in_set].astype(np.int64), obs_pt[in_set].astype(np.int64), obs_level[in_set].astype(np.int64)
    n_e = lk.size
    n_stale, n_dup, n_null = int(stale_frac * n_e), int(dup_frac * n_e), int(null_frac * n_e)
    xk, xp, xl = [lk], [lp], [ll]
    if n_pt and n_stale:
        sk, sp = rng.integers(0, n_cand, n_stale), rng.integers(0, n_pt, n_stale)
        listed = np.zeros((n_cand, n_pt), bool) if n_cand * n_pt <= 1 << 24 else None
        if listed is not None:
            listed[lk, lp] = True
            ok = ~listed[sk, sp]
        else:
            ok = ~np.isin(sk * n_pt + sp, lk * n_pt + lp)
        xk.append(sk[ok]); xp.append(sp[ok]); xl.append(rng.integers(0, n_levels, int(ok.sum())))
    if n_e and n_dup:
        d = rng.integers(0, n_e, n_dup)
        xk.append(lk[d]); xp.append(lp[d]); xl.append(rng.integers(0, n_levels, n_dup))
    xk.append(rng.integers(0, n_cand, n_null)); xp.append(np.full(n_null, -1)); xl.append(rng.integers(0, n_levels, n_null))
    lk, lp, ll = np.concatenate(xk), np.concatenate(xp), np.concatenate(xl)
    sh = rng.permutation(lk.size)
    so = sh[np.argsort(lk[sh], kind="stable")]
    lk, lp, ll = lk[so], lp[so], ll[so]
    list_off = np.concatenate([[0], np.cumsum(np.bincount(lk, minlength=n_cand))]).astype(np.int32)
    u = rng.random(n_cand)
    cand_flags = np.where(u < skip_frac, SKIP, np.where(u < skip_frac + not_erase_frac, NOT_ERASE, 0)).astype(np.uint8)
    return dict(n_cand=n_cand, n_all=n_all, n_pt=n_pt, n_levels=n_levels, cand_flags=cand_flags, list_off=list_off, list_pt=lp.astype(np.int32),
                list_level=ll.astype(np.uint8), pt_nobs=pt_nobs.astype(np.int32), pt_bad=pt_bad, obs_off=obs_off, obs_kf=obs_kf, obs_level=obs_level, obs_bad=obs_bad)


def profile_scene(size: str, seed: int = 0) -> dict:
    """A redundant-rich neighbourhood at SIZES[size]: n_cand candidates of about `slots` slots each"""
    n_cand, slots = SIZES[size]
    n_out = n_cand // 2
    # a point is listed by about 6.5 * n_cand / (n_cand + n_out) candidates, and about 2 % of the slots are stale, repeated or null
    n_pt = int(n_cand * slots / 1.02 / (6.5 * n_cand / (n_cand + n_out)))
    return make_scene(seed=seed, n_cand=n_cand, n_out=n_out, n_pt=n_pt, fine_frac=0.999, fine_obs=(5, 8), window=min(n_cand + n_out, 24), stale_frac=0.002,
                      dup_frac=0.002, null_frac=0.02, bad_kf_frac=0.02, bad_pt_frac=0.005, nobs_off_frac=0.0, skip_frac=0.04, not_erase_frac=0.04)


def reorder(sc: dict, walk_order) -> dict:
    """The same scene with the candidates walked in another order: walk_order[r] = the candidate of `sc` that is walked r-th.  Keyframe indices are renamed
    accordingly (new index r = old index walk_order[r]; the other observers keep theirs)."""
    n_cand, n_all = int(sc["n_cand"]), int(sc["n_all"])
    w = np.asarray(walk_order, np.int64)
    assert sorted(w.tolist()) == list(range(n_cand))
    old_of_new = np.concatenate([w, np.arange(n_cand, n_all)])
    new_of_old = np.empty(n_all, np.int64); new_of_old[old_of_new] = np.arange(n_all)
    loff = np.asarray(sc["list_off"], np.int64)
    seg = [np.arange(loff[k], loff[k + 1]) for k in w]
    idx = np.concatenate(seg) if seg else np.zeros(0, np.int64)
    out = dict(sc)
    out.update(cand_flags=np.asarray(sc["cand_flags"], np.uint8)[w], list_off=np.concatenate([[0], np.cumsum([s.size for s in seg])]).astype(np.int32),
               list_pt=np.asarray(sc["list_pt"], np.int32)[idx], list_level=np.asarray(sc["list_level"], np.uint8)[idx],
               obs_kf=new_of_old[np.asarray(sc["obs_kf"], np.int64)].astype(np.int32), old_of_new=old_of_new.astype(np.int32))
    return out
