"""PnP RANSAC of relocalisation candidates: cslam::PnPsolver (cslam/src/PnPSolver.cpp) and a round-robin of its iterate() over the candidates.

eval_hypotheses runs ccm_pnp_ransac_eval (one launch: H hypotheses of K candidates, each its inlier count, R | t in f64 and inlier mask); eval_hypotheses_host
runs the same lines (csrc/pnp_math.h) on the calling thread.  PnPRansac is the host mirror cslam::PnPRansacBatch (libccm_host.so, ccmh_pnp_*): next() returns
the next pose the reference's loop would return (candidate, Tcw, vbInliers in the frame's keypoint numbering), or None when every candidate is discarded.
Draws come from the C library's rand() through the calling thread's FIFO (sim3.draws_pending: the Sim3 and the PnP solvers of a thread share it), or from a
supplied array of raw rand() values.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from ._lib import CcmError, Context, _p, check, host, lib


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    h.ccmh_pnp_compute_pose.argtypes = [C.c_int] + [C.c_void_p] * 7
    h.ccmh_pnp_ransac_eval_host.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 6
    h.ccmh_pnp_check_inliers.argtypes = [C.c_int] + [C.c_void_p] * 7
    h.ccmh_pnp_refine.argtypes = [C.c_int] + [C.c_void_p] * 7
    h.ccmh_pnp_matrices.argtypes = [C.c_int] + [C.c_void_p] * 6
    h.ccmh_pnp_primitive.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 3
    h.ccmh_pnp_ransac_create.restype = C.c_void_p
    h.ccmh_pnp_ransac_create.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                                                                                 C.c_void_p, C.c_int64]
    h.ccmh_pnp_ransac_next.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]
    h.ccmh_pnp_ransac_iterate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    h.ccmh_pnp_ransac_stats.argtypes = [C.c_void_p, C.c_void_p]
    h.ccmh_pnp_ransac_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    h.ccmh_pnp_ransac_destroy.argtypes = [C.c_void_p]
    h.ccmh_pnp_ransac_destroy.restype = None
    return h


def max_errors(sigma2, th2: float = 5.991) -> np.ndarray:
    """mvMaxError = mvSigma2 * th2 (PnPSolver.cpp:146): a float product."""
    return np.asarray(sigma2, np.float32) * np.float32(th2)


@dataclass
class PnPCandidate:
    """The state PnPsolver's constructor gathers for one candidate keyframe (PnPSolver.cpp:57-100)."""
    P3Dw: np.ndarray            # mvP3Dw (N, 3) f32
    P2D: np.ndarray             # mvP2D (N, 2) f32
    sigma2: np.ndarray          # mvSigma2 (N,) f32
    cam: Sequence[float]        # fu fv uc vc (doubles in the reference)
    n_matches: int = -1         # vpMapPointMatches.size(); default N
    kp_idx: Optional[np.ndarray] = None   # mvKeyPointIndices; default 0 .. N-1
    meta: dict = field(default_factory=dict)

    @property
    def N(self) -> int:
        return int(np.asarray(self.sigma2).size)


def pack(cands: Sequence[PnPCandidate]):
    """CSR over the candidates: pt_off, P3Dw, P2D, sigma2, cam, n_matches, kp_idx as contiguous arrays."""
    pt_off = np.zeros(len(cands) + 1, np.int32)
    pt_off[1:] = np.cumsum([c.N for c in cands])
    cat = lambda xs, dt: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs]) if xs else np.zeros(0, dt), dt)
    P3 = cat([c.P3Dw for c in cands], np.float32)
    P2 = cat([c.P2D for c in cands], np.float32)
    s2 = cat([c.sigma2 for c in cands], np.float32)
    cam = np.ascontiguousarray(np.array([list(c.cam) for c in cands], np.float64).reshape(-1))
    nm = np.array([c.n_matches if c.n_matches >= 0 else c.N for c in cands], np.int32)
    kp = cat([c.kp_idx if c.kp_idx is not None else np.arange(c.N) for c in cands], np.int32)
    return pt_off, P3, P2, s2, cam, nm, kp


def _eval(call, cands, hyp_cand, hyp_idx, th2):
    pt_off, P3, P2, s2, cam, _, _ = pack(cands)
    me = np.ascontiguousarray(max_errors(s2, th2))
    hc = np.ascontiguousarray(hyp_cand, np.int32)
    hi = np.ascontiguousarray(hyp_idx, np.int32).reshape(-1)
    H = hc.size
    if hi.size != 4 * H:
        raise ValueError("hyp_idx must hold four indices per hypothesis")
    n_words = [(int(pt_off[c + 1] - pt_off[c]) + 31) // 32 for c in hc] if all(0 <= c < len(cands) for c in hc) else [0]
    n_inl = np.zeros(max(H, 1), np.int32)
    Rt = np.zeros((max(H, 1), 12), np.float64)
    mask_off = np.zeros(H + 1, np.int32)
    mask = np.full(max(sum(n_words), 1), 0xFFFFFFFF, np.uint32)   # the call writes every word, tail bits included
    call(len(cands), _p(pt_off), _p(P3), _p(P2), _p(me), _p(cam), int(H), _p(hc), _p(hi), _p(n_inl), _p(Rt), _p(mask_off), _p(mask))
    masks, tails = [], True
    for h in range(H):
        N = int(pt_off[hc[h] + 1] - pt_off[hc[h]])
        bits = np.unpackbits(mask[mask_off[h]:mask_off[h + 1]].astype("<u4").view(np.uint8), bitorder="little")
        tails = tails and not bits[N:].any()
        masks.append(bits[:N].astype(bool))
    if not tails:
        raise CcmError("a mask word holds bits beyond its candidate's N")
    return n_inl[:H], Rt[:H], masks


def eval_hypotheses(ctx: Context, cands: Sequence[PnPCandidate], hyp_cand, hyp_idx, th2: float = 5.991):
    """ccm_pnp_ransac_eval.  Returns (n_inl[H], Rt[H, 12] = R (9, row-major) t (3) in f64, list of H boolean inlier arrays of length N)."""
    def call(*a):
        check(lib().ccm_pnp_ransac_eval(ctx.handle, *a), ctx.handle)
    return _eval(call, cands, hyp_cand, hyp_idx, th2)


def eval_hypotheses_host(cands: Sequence[PnPCandidate], hyp_cand, hyp_idx, th2: float = 5.991):
    """The same through csrc/pnp_math.h on the calling thread (ccmh_pnp_ransac_eval_host)."""
    def call(*a):
        if _host().ccmh_pnp_ransac_eval_host(*a) != 0:
            raise CcmError("ccmh_pnp_ransac_eval_host: bad arguments")
    return _eval(call, cands, hyp_cand, hyp_idx, th2)


def compute_pose(pws, us, cam):
    """EPnP's compute_pose on n >= 4 correspondences (f64): (R 3x3, t 3, rep_errors[1..3], the chosen solution 1..3)."""
    pws = np.ascontiguousarray(pws, np.float64).reshape(-1, 3)
    us = np.ascontiguousarray(us, np.float64).reshape(-1, 2)
    cam = np.ascontiguousarray(cam, np.float64)
    R = np.zeros(9); t = np.zeros(3); rep = np.zeros(4); ch = C.c_int32(0)
    if _host().ccmh_pnp_compute_pose(pws.shape[0], _p(pws), _p(us), _p(cam), _p(R), _p(t), _p(rep), C.byref(ch)) != 0:
        raise CcmError("ccmh_pnp_compute_pose: bad arguments")
    return R.reshape(3, 3), t, rep[1:], ch.value


def check_inliers(cand: PnPCandidate, Rt, th2: float = 5.991):
    """CheckInliers of one pose (Rt = R row-major, t; f64): (mnInliersi, mvbInliersi, error2 per point as the reference's float)."""
    P3 = np.ascontiguousarray(cand.P3Dw, np.float32).reshape(-1); P2 = np.ascontiguousarray(cand.P2D, np.float32).reshape(-1)
    me = np.ascontiguousarray(max_errors(cand.sigma2, th2)); cam = np.ascontiguousarray(cand.cam, np.float64)
    Rt = np.ascontiguousarray(Rt, np.float64).reshape(-1)
    inl = np.zeros(max(cand.N, 1), np.uint8); e2 = np.zeros(max(cand.N, 1), np.float32)
    n = _host().ccmh_pnp_check_inliers(cand.N, _p(P3), _p(P2), _p(me), _p(cam), _p(Rt), _p(inl), _p(e2))
    if n < 0:
        raise CcmError("ccmh_pnp_check_inliers: bad arguments")
    return n, inl[:cand.N].astype(bool), e2[:cand.N]


def refine(cand: PnPCandidate, best_inliers, th2: float = 5.991):
    """Refine(): compute_pose on the correspondences of best_inliers, CheckInliers over all: (mnRefinedInliers, mvbRefinedInliers, Rt f64[12])."""
    P3 = np.ascontiguousarray(cand.P3Dw, np.float32).reshape(-1); P2 = np.ascontiguousarray(cand.P2D, np.float32).reshape(-1)
    me = np.ascontiguousarray(max_errors(cand.sigma2, th2)); cam = np.ascontiguousarray(cand.cam, np.float64)
    best = np.ascontiguousarray(best_inliers, np.uint8)
    Rt = np.zeros(12); inl = np.zeros(cand.N, np.uint8)
    n = _host().ccmh_pnp_refine(cand.N, _p(P3), _p(P2), _p(me), _p(cam), _p(best), _p(Rt), _p(inl))
    if n < 0:
        raise CcmError("ccmh_pnp_refine: bad arguments")
    return n, inl.astype(bool), Rt


class PnPRansac:
    """cslam::PnPRansacBatch over the given candidates.  device < 0 (or None): the host evaluator.  draws: raw rand() values to use instead of the C
    library's rand() (after the calling thread's FIFO).  Use it from the thread that created it."""

    def __init__(self, cands: Sequence[PnPCandidate], device: Optional[int] = 0, probability: float = 0.99, min_inliers: int = 8, max_iterations: int = 300,
                 min_set: int = 4, epsilon: float = 0.4, th2: float = 5.991, solver_iterations: int = 5, draws=None):
        pt_off, P3, P2, s2, cam, nm, kp = pack(cands)
        self._nm = nm
        d = None if draws is None else np.ascontiguousarray(draws, np.int32)
        self._h = _host().ccmh_pnp_ransac_create(-1 if device is None else int(device), len(cands), _p(pt_off), _p(P3), _p(P2), _p(s2), _p(cam), _p(nm), _p(kp),
                                                 float(probability), int(min_inliers), int(max_iterations), int(min_set), float(epsilon), float(th2),
                                                 int(solver_iterations), _p(d), 0 if d is None else int(d.size))
        if not self._h:
            raise CcmError("ccmh_pnp_ransac_create failed (bad arguments, min_set != 4, or no device)")

    def _result(self, rc, c, Tcw, inl, nin, flags):
        if rc == -1:
            raise CcmError("PnPRansac: the supplied draws ran out")
        if rc not in (0, 1):
            raise CcmError(f"PnPRansac failed ({rc})")
        if rc == 0:
            return None
        return dict(cand=c, Tcw=Tcw.reshape(4, 4).copy(), inliers=inl[:self._nm[c]].astype(bool), n_inliers=int(nin.value), refined=bool(flags[0]),
                    no_more=bool(flags[1]))

    def next(self):
        """The next pose of the round-robin: dict(cand, Tcw 4x4 f32, inliers bool[n_matches], n_inliers, refined, no_more), or None when every
        candidate is discarded."""
        cand = C.c_int32(-1); nin = C.c_int32(0); flags = np.zeros(2, np.int32)
        Tcw = np.zeros(16, np.float32); cap = int(self._nm.max()) if self._nm.size else 0
        inl = np.zeros(max(cap, 1), np.uint8)
        rc = _host().ccmh_pnp_ransac_next(self._h, C.byref(cand), _p(Tcw), _p(inl), cap, C.byref(nin), _p(flags))
        return self._result(rc, cand.value, Tcw, inl, nin, flags)

    def iterate(self, c: int, n: int):
        """One PnPsolver::iterate(n) of candidate c: (pose dict or None, bNoMore)."""
        nin = C.c_int32(0); flags = np.zeros(2, np.int32)
        Tcw = np.zeros(16, np.float32); cap = int(self._nm[c])
        inl = np.zeros(max(cap, 1), np.uint8)
        rc = _host().ccmh_pnp_ransac_iterate(self._h, int(c), int(n), _p(Tcw), _p(inl), cap, C.byref(nin), _p(flags))
        return self._result(rc, int(c), Tcw, inl, nin, flags), bool(flags[1])

    def stats(self):
        """(values taken from the draw source, hypotheses evaluated, evaluator calls, Refine computations)"""
        out = np.zeros(4, np.int64)
        _host().ccmh_pnp_ransac_stats(self._h, _p(out))
        return tuple(int(x) for x in out)

    def info(self, c: int):
        """(mnIterations, mRansacMaxIts, mRansacMinInliers, discarded) of candidate c"""
        out = np.zeros(4, np.int32)
        if _host().ccmh_pnp_ransac_info(self._h, int(c), _p(out)) != 0:
            raise CcmError("PnPRansac.info: no such candidate")
        return int(out[0]), int(out[1]), int(out[2]), bool(out[3])

    def close(self):
        if self._h:
            _host().ccmh_pnp_ransac_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
