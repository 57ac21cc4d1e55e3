"""ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs) (cslam/src/ORBmatcher.cpp:700-852) of LocalMapping::CreateNewMapPoints for all neighbours on
keyframes of a keyframe store that have their feature vector (KeyFrameStore.set_featvec).

pair_eval_resident runs ccm_tri_search_eval_resident: ONE launch for a list of jobs (key1, key2, has1, has2, F12, ex, ey).  pair_eval_host evaluates the same jobs on
the store's shadows through csrc/tri_search_math.h compiled for the host (libccm_host.so).  Both return the table (one 32-bit word per feature of every job's
keyframe 1, job after job; unpack() splits it), n_query, n_match and n_dist per job.  search_for_triangulation_batch is the host mirror
cslam::SearchForTriangulationBatch: one new keyframe against C neighbours, a sequence of resolve calls under the map-point flags of their moment.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional, Sequence

import numpy as np

from ._lib import CcmError, Context, _p, check, host, lib
from .bow_search import pack_masks
from .kfstore import KeyFrameStore

NOT_A_QUERY, NO_MATCH, MATCHED = 0, 1, 2
TH_LOW = 50
EPI_FLOATS = 11


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    V, I = C.c_void_p, C.c_int
    h.ccmh_tri_search_eval_resident_host.argtypes = [V, I] + [V] * 7 + [I] + [V] * 6
    h.ccmh_tri_search_create.restype = V
    h.ccmh_tri_search_create.argtypes = [V, I, C.c_int64, I] + [V] * 7 + [I, I]
    h.ccmh_tri_search_resolve.argtypes = [V, I, V, V, I, V]
    h.ccmh_tri_search_table.argtypes = [V] * 5
    h.ccmh_tri_search_n_reeval.restype = C.c_longlong
    h.ccmh_tri_search_n_reeval.argtypes = [V]
    h.ccmh_tri_search_destroy.restype = None
    h.ccmh_tri_search_destroy.argtypes = [V]
    return h


@functools.lru_cache(maxsize=None)
def _dev():
    l = lib()
    V, I = C.c_void_p, C.c_int
    l.ccm_tri_search_eval_resident.argtypes = [V, V, I] + [V] * 7 + [I] + [V] * 6
    return l


def pack_epi(F12, ex, ey) -> np.ndarray:
    """the 11 floats of one job: F12 row-major, ex, ey"""
    return np.concatenate([np.asarray(F12, np.float32).reshape(9), np.array([ex, ey], np.float32)])


def unpack(table) -> dict:
    """the fields of result words (tsm_pack of csrc/tri_search_math.h): status, bestIdx2 (-1: none), bestDist"""
    t = np.asarray(table, np.uint32)
    return dict(status=(t >> np.uint32(30)).astype(np.int32), idx=(t & np.uint32(0xFFFF)).astype(np.int32) - 1, dist=((t >> np.uint32(16)) & np.uint32(0xFF)).astype(np.int32))


def _job_args(jobs, sf2, sigma2_2):
    """jobs: [(key1, key2, has1, has2, F12, ex, ey)]"""
    jobs = list(jobs)
    k1 = np.array([j[0] for j in jobs], np.int64); k2 = np.array([j[1] for j in jobs], np.int64)
    off1, m1 = pack_masks([j[2] for j in jobs]); off2, m2 = pack_masks([j[3] for j in jobs])
    epi = np.concatenate([pack_epi(j[4], j[5], j[6]) for j in jobs]) if jobs else np.zeros(0, np.float32)
    sf = np.ascontiguousarray(sf2, np.float32); s2 = np.ascontiguousarray(sigma2_2, np.float32)
    assert sf.size == s2.size
    J = len(jobs)
    out = (np.zeros(int(off1[-1]), np.uint32), np.zeros(J, np.int32), np.zeros(J, np.int32), np.zeros(J, np.int32))
    return (k1, k2, off1, m1, off2, m2, epi, sf, s2), [J, _p(k1), _p(k2), _p(off1), _p(m1), _p(off2), _p(m2), _p(epi), int(sf.size), _p(sf), _p(s2)], out, off1


def _result(out, off1):
    return dict(table=out[0], n_query=out[1], n_match=out[2], n_dist=out[3], off=off1.astype(np.int64))


def pair_eval_resident(ctx: Context, store: KeyFrameStore, jobs, sf2, sigma2_2) -> dict:
    """ccm_tri_search_eval_resident on jobs = [(key1, key2, has1, has2, F12, ex, ey)]: table (job j's words at off[j] .. off[j + 1]), n_query, n_match, n_dist [J]"""
    keep, args, out, off1 = _job_args(jobs, sf2, sigma2_2)
    check(_dev().ccm_tri_search_eval_resident(ctx.handle, store.raw, *args, *[_p(x) for x in out]), ctx.handle)
    return _result(out, off1)


def pair_eval_resident_raw(ctx: Context, store: Optional[KeyFrameStore], J, key1, key2, has1_off, has1, has2_off, has2, job_epi, nlevels, sf2, sigma2_2, table, n_query,
                           n_match, n_dist) -> int:
    """the entry point's return code on raw arguments (None: a null pointer); the refusal tests call this"""
    a = [None if x is None else np.ascontiguousarray(x, dt) for x, dt in ((key1, np.int64), (key2, np.int64), (has1_off, np.int32), (has1, np.uint8), (has2_off, np.int32),
                                                                          (has2, np.uint8), (job_epi, np.float32), (sf2, np.float32), (sigma2_2, np.float32))]
    p = [_p(x) for x in a]
    return int(_dev().ccm_tri_search_eval_resident(ctx.handle, None if store is None else store.raw, int(J), *p[:7], int(nlevels), p[7], p[8], _p(table), _p(n_query),
                                                   _p(n_match), _p(n_dist)))


def pair_eval_host(store: KeyFrameStore, jobs, sf2, sigma2_2) -> dict:
    """the same jobs on the store's shadows on the calling thread (tri_search_eval_host of csrc/tri_search_math.h)"""
    keep, args, out, off1 = _job_args(jobs, sf2, sigma2_2)
    if _host().ccmh_tri_search_eval_resident_host(store.handle, *args, *[_p(x) for x in out]) != 0:
        raise CcmError("ccmh_tri_search_eval_resident_host: bad arguments, a key that is not live or a key without a feature vector")
    return _result(out, off1)


def pair_eval_host_raw(store: Optional[KeyFrameStore], J, key1, key2, has1_off, has1, has2_off, has2, job_epi, nlevels, sf2, sigma2_2, table, n_query, n_match, n_dist) -> int:
    """the host evaluator's return code on raw arguments (None: a null pointer)"""
    a = [None if x is None else np.ascontiguousarray(x, dt) for x, dt in ((key1, np.int64), (key2, np.int64), (has1_off, np.int32), (has1, np.uint8), (has2_off, np.int32),
                                                                          (has2, np.uint8), (job_epi, np.float32), (sf2, np.float32), (sigma2_2, np.float32))]
    p = [_p(x) for x in a]
    return int(_host().ccmh_tri_search_eval_resident_host(None if store is None else store.handle, int(J), *p[:7], int(nlevels), p[7], p[8], _p(table), _p(n_query),
                                                          _p(n_match), _p(n_dist)))


class Batch:
    """cslam::SearchForTriangulationBatch: the constructor makes the one device call (host=True or a host-only store: the host evaluation)"""

    def __init__(self, store: KeyFrameStore, key1: int, keys2, has1, has2: Sequence, epi: Sequence, sigma2_2, sf2, check_orientation: bool, host: bool = False):
        keys2 = np.ascontiguousarray(np.asarray(list(keys2), np.int64).reshape(-1))
        self.C = int(keys2.size)
        h1 = np.ascontiguousarray(np.asarray(has1, np.uint8).reshape(-1))
        self.N1 = int(h1.size)
        off2, m2 = pack_masks(has2)
        e = np.concatenate([pack_epi(*x) for x in epi]) if self.C else np.zeros(0, np.float32)
        assert e.size == EPI_FLOATS * self.C
        sf = np.ascontiguousarray(sf2, np.float32); s2 = np.ascontiguousarray(sigma2_2, np.float32)
        self._h = _host().ccmh_tri_search_create(store.handle, -1 if host else store.device, int(key1), self.C, _p(keys2), _p(h1), _p(off2), _p(m2), _p(e), _p(s2), _p(sf),
                                                 int(sf.size), int(bool(check_orientation)))
        if not self._h:
            raise CcmError("ccmh_tri_search_create failed (bad arguments, a key that is not live or has no feature vector, or a device error)")

    def resolve(self, j: int, has1_now=None, has2_now=None):
        """(nmatches, matches12) of neighbour j under the flags of this moment (None: the build's)"""
        a = None if has1_now is None else np.ascontiguousarray(has1_now, np.uint8)
        b = None if has2_now is None else np.ascontiguousarray(has2_now, np.uint8)
        m = np.zeros(self.N1, np.int32)
        n = _host().ccmh_tri_search_resolve(self._h, int(j), _p(a), _p(b), self.N1, _p(m))
        if n < 0:
            raise CcmError(f"ccmh_tri_search_resolve: {n}")
        return n, m

    def predicted(self, j: int) -> np.ndarray:
        """(idx1, idx2) pairs of neighbour j under the flags of the build, ascending idx1: vMatchedPairs"""
        _, m = self.resolve(j)
        i = np.flatnonzero(m >= 0)
        return np.stack([i, m[i]], 1).astype(np.int32)

    def tables(self) -> dict:
        table = np.zeros(self.N1 * self.C, np.uint32); nq = np.zeros(self.C, np.int32); nm = np.zeros(self.C, np.int32); nd = np.zeros(self.C, np.int32)
        _host().ccmh_tri_search_table(self._h, _p(table), _p(nq), _p(nm), _p(nd))
        return dict(table=table, n_query=nq, n_match=nm, n_dist=nd)

    @property
    def reevaluated(self) -> int:
        return int(_host().ccmh_tri_search_n_reeval(self._h))

    def close(self):
        if self._h:
            _host().ccmh_tri_search_destroy(self._h)
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


def search_for_triangulation_batch(store: KeyFrameStore, key1: int, keys2, has1, has2: Sequence, epi: Sequence, sigma2_2, sf2, check_orientation: bool,
                                   host: bool = False) -> dict:
    """SearchForTriangulation(key1, keys2[j]) for every neighbour from ONE device call, each resolved under the flags of the build: nmatches[C], matches12[C] (one
    entry per feature of key1: the feature of keys2[j] or -1), reevaluated, and the table / counters of the one evaluation"""
    with Batch(store, key1, keys2, has1, has2, epi, sigma2_2, sf2, check_orientation, host) as b:
        nm, m12 = [], []
        for j in range(b.C):
            n, m = b.resolve(j)
            nm.append(n); m12.append(m)
        return dict(nmatches=nm, matches12=m12, reevaluated=b.reevaluated, **b.tables())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# generator (numpy only; nothing here touches the device)
# ---------------------------------------------------------------------------------------------------------------------------------------------
PROFILE_SIZES = {"20x1000": dict(neighbours=20, features=1000), "20x2000": dict(neighbours=20, features=2000), "5x1000": dict(neighbours=5, features=1000)}


def epipolar_of(K4, t2) -> tuple:
    """(F12, ex, ey) of a new keyframe at the identity pose and a neighbour with the identity rotation and translation t2 (T2w): F12 = K^-T [t]x K^-1 with
    t = -t2 rounded to f32, and the epipole of :708-714 in f32 (C2 = t2)"""
    K4 = np.asarray(K4, np.float32); t2 = np.asarray(t2, np.float32)
    Kk = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1]], np.float64)
    t = -t2.astype(np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F12 = (np.linalg.inv(Kk).T @ tx @ np.linalg.inv(Kk)).astype(np.float32)
    invz = np.float32(1.0) / t2[2]
    ex = np.float32(np.float32(K4[0] * t2[0]) * invz) + K4[2]
    ey = np.float32(np.float32(K4[1] * t2[1]) * invz) + K4[3]
    return F12, np.float32(ex), np.float32(ey)


def profile_scene(neighbours: int, features: int, n_nodes: int = 100, seed: int = 0, has_share: float = 0.5, K4=(458.654, 457.296, 367.215, 248.375),
                  nlevels: int = 8) -> dict:
    """One CreateNewMapPoints: a new keyframe of `features` features over n_nodes vocabulary nodes at the identity pose and `neighbours` keyframes that see the
    same scene from a translated pose.  Scene points at depths 2 .. 8 m are projected into both views, so every true match lies on its epipolar line (half a pixel
    of noise); F12 and the epipole of every neighbour follow from its pose (epipolar_of).  Descriptors: 6 % of the bits flipped, shuffled; nine words in ten fall
    into the same node, 3 % are stopped.  A share of the features already holds a map point.  kfs[0] is the new keyframe."""
    rng = np.random.default_rng(seed)
    K4 = np.asarray(K4, np.float32)
    base = rng.integers(0, 256, (features, 32), dtype=np.uint8)
    node0 = rng.integers(0, n_nodes, features)
    ang0 = rng.uniform(0, 360, features).astype(np.float32)
    oct0 = np.minimum(rng.geometric(0.45, features) - 1, nlevels - 1).astype(np.uint8)
    uv0 = np.stack([rng.uniform(20, 732, features), rng.uniform(20, 460, features)], 1)
    depth = rng.uniform(2.0, 8.0, features)
    X = np.stack([(uv0[:, 0] - K4[2]) / K4[0] * depth, (uv0[:, 1] - K4[3]) / K4[1] * depth, depth], 1)

    def fv_of(node_of):
        nodes = np.unique(node_of[node_of >= 0])
        order = np.argsort(node_of, kind="stable")
        order = order[node_of[order] >= 0]
        off = np.concatenate([[0], np.cumsum([(node_of == nd).sum() for nd in nodes])])
        return nodes.astype(np.int32), off.astype(np.int32), order.astype(np.int32)

    def view(k):
        t2 = np.zeros(3, np.float32) if k == 0 else np.array([-0.10 - 0.01 * k, 0.01 * (k % 3), 0.02], np.float32)
        perm = rng.permutation(features) if k else np.arange(features)
        bits = np.unpackbits(base[perm], axis=1)
        desc = np.packbits(bits ^ (rng.random(bits.shape) < (0.06 if k else 0.0)), axis=1)
        node = node0[perm].copy()
        moved = rng.random(features) < (0.1 if k else 0.0)
        node[moved] = rng.integers(0, n_nodes, int(moved.sum()))
        node[rng.random(features) < 0.03] = -1
        Xc = X[perm] + t2.astype(np.float64)
        xy = np.stack([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3]], 1) + (rng.normal(0, 0.5, (features, 2)) if k else 0.0)
        angle = (ang0[perm] + rng.normal(0, 2.0, features).astype(np.float32)) % np.float32(360.0)
        out = dict(desc=np.ascontiguousarray(desc), angle=angle.astype(np.float32), fv=fv_of(node), xy=np.ascontiguousarray(xy, np.float32), octave=oct0[perm].copy(),
                   has=(rng.random(features) < has_share).astype(np.uint8), t2=t2)
        if k:
            out["F12"], out["ex"], out["ey"] = epipolar_of(K4, t2)
        return out
    sf = (np.float32(1.2) ** np.arange(nlevels)).astype(np.float32)
    return dict(kfs=[view(k) for k in range(neighbours + 1)], n_nodes=n_nodes, K4=K4, scale_factors=sf, level_sigma2=(sf * sf).astype(np.float32))
