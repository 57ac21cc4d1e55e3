"""Sim3 RANSAC of loop and map-match candidates: cslam::Sim3Solver (cslam/src/Sim3Solver.cpp) and the round-robin of LoopFinder / MapMatcher::ComputeSim3.

eval_hypotheses runs ccm_sim3_ransac_eval (one launch: H hypotheses of K candidates, each its inlier count, R / t / s and inlier mask).  Sim3Ransac is the
host mirror cslam::Sim3RansacBatch (libccm_host.so, ccmh_sim3_*): next() returns the next Sim3 the reference's loop would return (candidate, R, t, s,
vbInliers in the candidate's mN1 numbering), or None when every candidate is discarded.  Draws come from the C library's rand() through the calling
thread's FIFO (draws_pending), or from a supplied array of raw rand() values.
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
    h.ccmh_sim3_ransac_create.restype = C.c_void_p
    h.ccmh_sim3_ransac_create.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 9 + [C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                                                                  C.c_void_p, C.c_int64]
    h.ccmh_sim3_ransac_next.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    h.ccmh_sim3_ransac_stats.argtypes = [C.c_void_p, C.c_void_p]
    h.ccmh_sim3_ransac_destroy.argtypes = [C.c_void_p]
    h.ccmh_sim3_ransac_destroy.restype = None
    h.ccmh_sim3_draws_pending.argtypes = [C.c_void_p, C.c_int]
    h.ccmh_sim3_draws_clear.restype = None
    h.ccmh_sim3_solver_iterate.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4
    return h


def max_error_thresholds(sigma2) -> np.ndarray:
    """mvnMaxError = 9.210 * mvLevelSigma2[octave], stored in a std::vector<size_t>: the double product truncated."""
    return (9.210 * np.asarray(sigma2, np.float32).astype(np.float64)).astype(np.uint32)


@dataclass
class Sim3Candidate:
    """The state Sim3Solver's constructor gathers for one candidate keyframe (Sim3Solver.cpp:5-92)."""
    X1: np.ndarray              # mvX3Dc1 (N, 3) f32: Rcw1 * X + tcw1
    X2: np.ndarray              # mvX3Dc2
    thr1: np.ndarray            # mvnMaxError1 (N,) uint32
    thr2: np.ndarray
    K1: Sequence[float]         # fx fy cx cy of pKF1->mK
    K2: Sequence[float]
    n1: int = -1                # mN1 = vpMatched12.size(); default N
    idx1: Optional[np.ndarray] = None   # mvnIndices1; default 0 .. N-1
    meta: dict = field(default_factory=dict)

    @property
    def N(self) -> int:
        return int(np.asarray(self.X1).shape[0])


def pack(cands: Sequence[Sim3Candidate]):
    """CSR over the candidates: pt_off, X1, X2, K1, K2, thr1, thr2, n1, idx1 as contiguous arrays."""
    n = [c.N for c in cands]
    pt_off = np.zeros(len(cands) + 1, np.int32)
    pt_off[1:] = np.cumsum(n)
    cat = lambda xs, dt, shape: np.ascontiguousarray(np.concatenate([np.asarray(x, dt).reshape(shape) for x in xs]) if xs else np.zeros(0, dt), dt)
    X1 = cat([c.X1 for c in cands], np.float32, (-1,))
    X2 = cat([c.X2 for c in cands], np.float32, (-1,))
    t1 = cat([c.thr1 for c in cands], np.uint32, (-1,))
    t2 = cat([c.thr2 for c in cands], np.uint32, (-1,))
    K1 = np.ascontiguousarray(np.array([list(c.K1) for c in cands], np.float32).reshape(-1))
    K2 = np.ascontiguousarray(np.array([list(c.K2) for c in cands], np.float32).reshape(-1))
    n1 = np.array([c.n1 if c.n1 >= 0 else c.N for c in cands], np.int32)
    idx1 = cat([c.idx1 if c.idx1 is not None else np.arange(c.N) for c in cands], np.int32, (-1,))
    return pt_off, X1, X2, K1, K2, t1, t2, n1, idx1


def eval_hypotheses(ctx: Context, cands: Sequence[Sim3Candidate], hyp_cand, hyp_idx, fix_scale: bool = False):
    """ccm_sim3_ransac_eval.  Returns (n_inl[H], rts[H, 13] = R (9) t (3) s, list of H boolean inlier arrays (one per hypothesis, length N))."""
    pt_off, X1, X2, K1, K2, t1, t2, _, _ = pack(cands)
    hc = np.ascontiguousarray(hyp_cand, np.int32)
    hi = np.ascontiguousarray(hyp_idx, np.int32).reshape(-1)
    H = hc.size
    if hi.size != 3 * H:
        raise ValueError("hyp_idx must hold three indices per hypothesis")
    n_words = [(int(pt_off[c + 1] - pt_off[c]) + 31) // 32 for c in hc] if all(0 <= c < len(cands) for c in hc) else [0]
    n_inl = np.zeros(max(H, 1), np.int32)
    rts = np.zeros((max(H, 1), 13), np.float32)
    mask_off = np.zeros(H + 1, np.int32)
    mask = np.zeros(max(sum(n_words), 1), np.uint32)
    check(lib().ccm_sim3_ransac_eval(ctx.handle, len(cands), _p(pt_off), _p(X1), _p(X2), _p(K1), _p(K2), _p(t1), _p(t2), int(H), _p(hc), _p(hi),
                                     int(bool(fix_scale)), _p(n_inl), _p(rts), _p(mask_off), _p(mask)), ctx.handle)
    masks = []
    for h in range(H):
        N = int(pt_off[hc[h] + 1] - pt_off[hc[h]])
        words = mask[mask_off[h]:mask_off[h + 1]]
        bits = np.unpackbits(words.astype("<u4").view(np.uint8), bitorder="little")[:N].astype(bool)
        masks.append(bits)
    return n_inl[:H], rts[:H], masks


class Sim3Ransac:
    """cslam::Sim3RansacBatch: the vpSim3Solvers loop of LoopFinder::ComputeSim3 over the given candidates.  draws: raw rand() values to use instead
    of the C library's rand() (after the calling thread's FIFO).  Use it from the thread that created it."""

    def __init__(self, cands: Sequence[Sim3Candidate], device: int = 0, probability: float = 0.99, min_inliers: int = 6, max_iterations: int = 300,
                 solver_iterations: int = 5, fix_scale: bool = False, draws=None):
        pt_off, X1, X2, K1, K2, t1, t2, n1, idx1 = pack(cands)
        self._keep = (pt_off, X1, X2, K1, K2, t1, t2, n1, idx1)
        self._n1 = n1
        d = None if draws is None else np.ascontiguousarray(draws, np.int32)
        self._h = _host().ccmh_sim3_ransac_create(int(device), len(cands), _p(pt_off), _p(X1), _p(X2), _p(K1), _p(K2), _p(t1), _p(t2), _p(n1), _p(idx1),
                                                  float(probability), int(min_inliers), int(max_iterations), int(solver_iterations), int(bool(fix_scale)),
                                                  _p(d), 0 if d is None else int(d.size))
        if not self._h:
            raise CcmError("ccmh_sim3_ransac_create failed (bad arguments or no device)")

    def next(self):
        """(candidate, R 3x3, t 3, s, vbInliers bool[mN1], nInliers) of the next Sim3, or None when every candidate is discarded."""
        cand = C.c_int32(-1); nin = C.c_int32(0)
        R = np.zeros(9, np.float32); t = np.zeros(3, np.float32); s = np.zeros(1, np.float32)
        cap = int(self._n1.max()) if self._n1.size else 0
        inl = np.zeros(max(cap, 1), np.uint8)
        rc = _host().ccmh_sim3_ransac_next(self._h, C.byref(cand), _p(R), _p(t), _p(s), _p(inl), cap, C.byref(nin))
        if rc == 0:
            return None
        if rc == -1:
            raise CcmError("Sim3Ransac: the supplied draws ran out")
        if rc != 1:
            raise CcmError(f"ccmh_sim3_ransac_next failed ({rc})")
        c = cand.value
        return c, R.reshape(3, 3).copy(), t.copy(), float(s[0]), inl[:self._n1[c]].astype(bool), nin.value

    def stats(self):
        """(values taken from the draw source, hypotheses evaluated, device passes)"""
        out = np.zeros(3, np.int64)
        _host().ccmh_sim3_ransac_stats(self._h, _p(out))
        return tuple(int(x) for x in out)

    def close(self):
        if self._h:
            _host().ccmh_sim3_ransac_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sim3Solver:
    """One cslam::Sim3Solver as the drop-in shim/Sim3Solver_hip.cpp runs it: iterate(n) evaluates its at most n hypotheses in one launch
    (ccmh_sim3_solver_iterate), drawing from the C library's rand() through the calling thread's FIFO."""

    def __init__(self, cand: Sim3Candidate, device: int = 0, probability: float = 0.99, min_inliers: int = 6, max_iterations: int = 300,
                 fix_scale: bool = False):
        self.c, self.device, self.fix_scale, self.min_inliers = cand, int(device), bool(fix_scale), int(min_inliers)
        N = cand.N
        self._a = [np.ascontiguousarray(np.asarray(x, dt).reshape(-1)) for x, dt in ((cand.X1, np.float32), (cand.X2, np.float32), (cand.K1, np.float32),
                                                                                     (cand.K2, np.float32), (cand.thr1, np.uint32), (cand.thr2, np.uint32))]
        if N >= min_inliers and N > 0:   # SetRansacParameters (Sim3Solver.cpp:94-118)
            eps = np.float32(np.float32(min_inliers) / np.float32(N))
            n_it = 1 if min_inliers == N else int(np.ceil(np.log(1 - probability) / np.log(1 - float(eps) ** 3)))
            self.max_iterations = max(1, min(n_it, int(max_iterations)))
        else:
            self.max_iterations = 1
        self.state = np.zeros(2, np.int32)   # mnIterations, mnBestInliers

    def iterate(self, n: int):
        """(success, bNoMore, best, n_inliers): best = (R, t, s, inlier flags over the N correspondences) of the last hypothesis that moved the
        best estimate in this call, or None."""
        N = self.c.N
        rts = np.zeros(13, np.float32); mask = np.zeros((N + 31) // 32 + 1, np.uint32); flags = np.zeros(4, np.int32)
        rc = _host().ccmh_sim3_solver_iterate(self.device, N, *(_p(a) for a in self._a), int(self.fix_scale), self.min_inliers, self.max_iterations, int(n),
                                              _p(self.state), _p(rts), _p(mask), _p(flags))
        if rc != 0:
            raise CcmError(f"ccmh_sim3_solver_iterate failed ({rc})")
        best = None
        if flags[2]:
            inl = np.unpackbits(mask.astype("<u4").view(np.uint8), bitorder="little")[:N].astype(bool)
            best = (rts[:9].reshape(3, 3).copy(), rts[9:12].copy(), float(rts[12]), inl)
        return bool(flags[0]), bool(flags[1]), best, int(flags[3])


def draws_pending() -> np.ndarray:
    """The calling thread's FIFO of rand() values drawn for hypotheses after a Sim3 event, front first."""
    n = _host().ccmh_sim3_draws_pending(None, 0)
    out = np.zeros(max(n, 1), np.int32)
    n = _host().ccmh_sim3_draws_pending(_p(out), n)
    return out[:n].copy()


def clear_draws() -> None:
    _host().ccmh_sim3_draws_clear()
