"""Keyframe database of place recognition (ccm_kfdb_* of the C ABI): cslam::KeyFrameDatabase (cslam/src/Database.cpp).

KeyFrameDatabase.add / erase / clear and the raw phase-1 table of a query (which keyframes share enough words with the query, in the reference's
lKFsSharingWords order, with their shared-word counts and L1 scores) run on the device; detect_loop_candidates / detect_map_match_candidates /
detect_relocalization_candidates add phase 2 (covisibility accumulation, Database.cpp:148-201) through the C++ host mirror (libccm_host.so,
ccm_slam_amd/host/kfdb_resolve.h).  A BowVector is a pair (word ids ascending int32, values f64).  Keys are int64; `group` is the client id.
One database may be queried from several threads at once, each with its own Context.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Dict, Iterable, Optional, Sequence

import numpy as np

from ._lib import CcmError, Context, _p, check, host, lib

class KfdbFilter(C.Structure):
    _fields_ = [("self_key", C.c_int64), ("allow", C.c_void_p), ("n_allow", C.c_int), ("exclude", C.c_void_p), ("n_exclude", C.c_int),
                ("exclude_groups", C.c_uint64)]


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    h.ccmh_kfdb_detect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return h


def _bow(word, value):
    w = np.ascontiguousarray(word, np.int32)
    v = np.ascontiguousarray(value, np.float64)
    if w.shape != v.shape or w.ndim != 1:
        raise ValueError("a BowVector is two 1-D arrays of the same length")
    return w, v


def _keys(keys) -> np.ndarray:
    return np.ascontiguousarray(np.fromiter((int(k) for k in keys), np.int64) if not isinstance(keys, np.ndarray) else keys, np.int64)


def group_mask(clients: Iterable[int]) -> int:
    """pMap->msuAssClients as the exclude_groups bit mask (client ids < 64)."""
    m = 0
    for c in clients:
        if 0 <= int(c) < 64:
            m |= 1 << int(c)
    return m


class KeyFrameDatabase:
    def __init__(self, ctx: Context, n_words: int, log_capacity: int = 0):
        self.ctx = ctx
        self._h = C.c_void_p()
        lib().ccm_kfdb_destroy.restype = None
        check(lib().ccm_kfdb_create(ctx.handle, int(n_words), int(log_capacity), C.byref(self._h)), ctx.handle)
        ctx.adopt(self)

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().ccm_kfdb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _c(self, ctx):
        return (ctx or self.ctx).handle

    def add(self, key: int, group: int, word, value, ctx: Optional[Context] = None):
        w, v = _bow(word, value)
        check(lib().ccm_kfdb_add(self._h, self._c(ctx), C.c_int64(int(key)), C.c_int32(int(group)), w.size, _p(w), _p(v)), self._c(ctx))

    def erase(self, key: int, ctx: Optional[Context] = None):
        check(lib().ccm_kfdb_erase(self._h, self._c(ctx), C.c_int64(int(key))), self._c(ctx))

    def clear(self, ctx: Optional[Context] = None):
        check(lib().ccm_kfdb_clear(self._h, self._c(ctx)), self._c(ctx))

    def query(self, word, value, self_key: int = -1, allow: Optional[Sequence[int]] = None, exclude: Sequence[int] = (), exclude_groups: int = 0,
              ctx: Optional[Context] = None, cap: int = 256) -> dict:
        """Phase 1 of one query (ccm_kfdb_query): dict(key, count, score (f32), score64, n_sharing, max_common, generation), rows in
        lKFsSharingWords order."""
        w, v = _bow(word, value)
        al = _keys(allow) if allow is not None else None
        ex = _keys(exclude)
        if al is not None and al.size == 0:
            al = np.zeros(1, np.int64)[:0]   # an empty allow list admits nothing (a non-NULL pointer with n_allow = 0)
        f = KfdbFilter(int(self_key), al.ctypes.data if al is not None else None, 0 if al is None else al.size, _p(ex) if ex.size else None, ex.size,
                       C.c_uint64(int(exclude_groups)))
        while True:
            key = np.empty(max(cap, 1), np.int64); cnt = np.empty(max(cap, 1), np.int32)
            sc = np.empty(max(cap, 1), np.float32); s64 = np.empty(max(cap, 1), np.float64)
            n, ns, mc, gen = C.c_int(), C.c_int(), C.c_int(), C.c_uint64()
            check(lib().ccm_kfdb_query(self._h, self._c(ctx), w.size, _p(w), _p(v), C.byref(f), cap, _p(key), _p(cnt), _p(sc), _p(s64),
                                       C.byref(n), C.byref(ns), C.byref(mc), C.byref(gen)), self._c(ctx))
            if n.value <= cap:
                break
            cap = n.value
        m = n.value
        return dict(key=key[:m].copy(), count=cnt[:m].copy(), score=sc[:m].copy(), score64=s64[:m].copy(), n_sharing=ns.value, max_common=mc.value,
                    generation=gen.value)

    def score(self, word, value, keys, ctx: Optional[Context] = None) -> np.ndarray:
        """voc.score(q, kf) in f64 for every listed key (ccm_kfdb_score)."""
        w, v = _bow(word, value)
        k = _keys(keys)
        out = np.empty(max(k.size, 1), np.float64)
        check(lib().ccm_kfdb_score(self._h, self._c(ctx), w.size, _p(w), _p(v), _p(k), k.size, _p(out)), self._c(ctx))
        return out[:k.size]

    # phase 1 + phase 2 through the host mirror ---------------------------------------------------------------------------------
    def _detect(self, kind, word, value, min_score, neighbours, self_key=-1, allow=None, exclude=(), exclude_groups=0):
        w, v = _bow(word, value)
        al = _keys(allow) if allow is not None else np.zeros(0, np.int64)
        ex = _keys(exclude)
        nb = neighbours or {}
        nk = np.fromiter(nb.keys(), np.int64, len(nb))
        noff = np.zeros(len(nb) + 1, np.int32)
        noff[1:] = np.cumsum([len(nb[k]) for k in nb]) if nb else []
        nl = np.ascontiguousarray(np.concatenate([np.asarray(nb[k], np.int64) for k in nb]) if nb else np.zeros(0, np.int64), np.int64)
        cap = 1024
        while True:
            out = np.empty(cap, np.int64)
            n = _host().ccmh_kfdb_detect(self._h, self.ctx.device, kind, w.size, _p(w), _p(v), float(min_score), int(self_key), _p(al) if al.size else None,
                                         al.size if allow is not None else -1, _p(ex) if ex.size else None, ex.size, int(exclude_groups), nk.size, _p(nk),
                                         _p(noff), _p(nl) if nl.size else None, _p(out), cap)
            if n < 0:
                raise CcmError(f"ccmh_kfdb_detect failed ({n})")
            if n <= cap:
                return [int(k) for k in out[:n]]
            cap = n

    def detect_loop_candidates(self, key, word, value, min_score: float, map_keys: Optional[Sequence[int]], connected: Sequence[int],
                               neighbours: Dict[int, Sequence[int]]):
        """DetectLoopCandidates (Database.cpp:72-202): map_keys = GetMmpKeyFrames() keys (None: every keyframe), connected = GetConnectedKeyFrames(),
        neighbours[key] = GetBestCovisibilityKeyFrames(10)."""
        return self._detect(0, word, value, min_score, neighbours, self_key=key, allow=map_keys, exclude=connected)

    def detect_map_match_candidates(self, word, value, min_score: float, ass_clients: Iterable[int], neighbours: Dict[int, Sequence[int]]):
        """DetectMapMatchCandidates (Database.cpp:204-327): ass_clients = pMap->msuAssClients."""
        return self._detect(1, word, value, min_score, neighbours, exclude_groups=group_mask(ass_clients))

    def detect_relocalization_candidates(self, word, value, neighbours: Dict[int, Sequence[int]]):
        """DetectRelocalizationCandidates (Database.cpp:329-439); neighbours that are listed but not scored contribute 0.0f (kfdb_resolve.h)."""
        return self._detect(2, word, value, 0.0, neighbours)
