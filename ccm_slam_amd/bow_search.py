"""ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) (cslam/src/ORBmatcher.cpp:565-698) of LoopFinder::ComputeSim3 / MapMatcher::ComputeSim3 for all candidates
on keyframes of a keyframe store that have their feature vector (KeyFrameStore.set_featvec).

pair_eval_resident runs ccm_bow_pair_eval_resident: ONE launch for a list of jobs (key1, key2, live1, live2), evaluated on the INITIAL vbMatched2.  pair_eval_host
evaluates the same jobs on the store's shadows through csrc/bow_search_math.h compiled for the host (libccm_host.so).  Both return the table (one 64-bit word per
feature of every job's keyframe 1, job after job; unpack() splits it), n_query and n_dist per job.  search_by_bow_batch is the host mirror
cslam::SearchByBoWBatch: one current keyframe against C candidates, matches12 and nmatches per candidate as SearchByBoW returns them, and how many queries the
replay of the claims evaluated again.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Sequence

import numpy as np

from ._lib import CcmError, Context, _p, check, host, lib
from .kfstore import KeyFrameStore

NOT_A_QUERY, NO_CANDIDATE, EVALUATED = 0, 1, 2
TH_LOW = 50


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    V, I, F = C.c_void_p, C.c_int, C.c_float
    h.ccmh_bow_pair_eval_resident_host.argtypes = [V, I] + [V] * 9
    h.ccmh_bow_batch_create.restype = V
    h.ccmh_bow_batch_create.argtypes = [V, I, C.c_int64, I, V, V, V, V, F, I]
    h.ccmh_bow_batch_result.argtypes = [V, I, I, V]
    h.ccmh_bow_batch_table.argtypes = [V] * 4
    h.ccmh_bow_batch_n_reeval.restype = C.c_longlong
    h.ccmh_bow_batch_n_reeval.argtypes = [V]
    h.ccmh_bow_batch_destroy.restype = None
    h.ccmh_bow_batch_destroy.argtypes = [V]
    return h


@functools.lru_cache(maxsize=None)
def _dev():
    l = lib()
    V, I = C.c_void_p, C.c_int
    l.ccm_bow_pair_eval_resident.argtypes = [V, V, I] + [V] * 9
    return l


def pack_masks(masks: Sequence):
    """(off[J + 1], bytes) of one mask per job"""
    m = [np.ascontiguousarray(np.asarray(x, np.uint8).reshape(-1)) for x in masks]
    off = np.zeros(len(m) + 1, np.int32)
    off[1:] = np.cumsum([x.size for x in m])
    return off, (np.concatenate(m) if m else np.zeros(0, np.uint8))


def unpack(table) -> dict:
    """the fields of result words (bsm_pack of csrc/bow_search_math.h): status, bestDist1, bestIdx2 (-1: none), bestDist2, and the position of the query's node in
    keyframe 2's node list"""
    t = np.asarray(table, np.uint64)
    return dict(status=(t >> np.uint64(62)).astype(np.int32), d1=((t >> np.uint64(16)) & np.uint64(0x1FF)).astype(np.int32),
                idx=(t & np.uint64(0xFFFF)).astype(np.int32) - 1, d2=((t >> np.uint64(25)) & np.uint64(0x1FF)).astype(np.int32),
                node2=((t >> np.uint64(34)) & np.uint64(0xFFFF)).astype(np.int32))


def _job_args(jobs):
    """jobs: [(key1, key2, live1, live2)]"""
    jobs = list(jobs)
    k1 = np.array([j[0] for j in jobs], np.int64); k2 = np.array([j[1] for j in jobs], np.int64)
    off1, m1 = pack_masks([j[2] for j in jobs]); off2, m2 = pack_masks([j[3] for j in jobs])
    J = len(jobs)
    out = (np.zeros(int(off1[-1]), np.uint64), np.zeros(J, np.int32), np.zeros(J, np.int32))
    return (k1, k2, off1, m1, off2, m2), [J, _p(k1), _p(k2), _p(off1), _p(m1), _p(off2), _p(m2)], out, off1


def _result(out, off1):
    return dict(table=out[0], n_query=out[1], n_dist=out[2], off=off1.astype(np.int64))


def pair_eval_resident(ctx: Context, store: KeyFrameStore, jobs) -> dict:
    """ccm_bow_pair_eval_resident on jobs = [(key1, key2, live1, live2)]: table (job j's words at off[j] .. off[j + 1]), n_query[J], n_dist[J]"""
    keep, args, out, off1 = _job_args(jobs)
    check(_dev().ccm_bow_pair_eval_resident(ctx.handle, store.raw, *args, _p(out[0]), _p(out[1]), _p(out[2])), ctx.handle)
    return _result(out, off1)


def pair_eval_resident_raw(ctx: Context, store: KeyFrameStore, J, key1, key2, live1_off, live1, live2_off, live2, table, n_query, n_dist) -> int:
    """the entry point's return code on raw arguments (None: a null pointer); the refusal tests call this"""
    a = [None if x is None else np.ascontiguousarray(x, dt) for x, dt in ((key1, np.int64), (key2, np.int64), (live1_off, np.int32), (live1, np.uint8),
                                                                          (live2_off, np.int32), (live2, np.uint8))]
    return int(_dev().ccm_bow_pair_eval_resident(ctx.handle, None if store is None else store.raw, int(J), *[_p(x) for x in a], _p(table), _p(n_query), _p(n_dist)))


def pair_eval_host(store: KeyFrameStore, jobs) -> dict:
    """the same jobs on the store's shadows on the calling thread (bow_pair_eval_host of csrc/bow_search_math.h)"""
    keep, args, out, off1 = _job_args(jobs)
    if _host().ccmh_bow_pair_eval_resident_host(store.handle, *args, _p(out[0]), _p(out[1]), _p(out[2])) != 0:
        raise CcmError("ccmh_bow_pair_eval_resident_host: bad arguments, a key that is not live or a key without a feature vector")
    return _result(out, off1)


def search_by_bow_batch(store: KeyFrameStore, key1: int, keys2, live1, live2: Sequence, nnratio: float, check_orientation: bool, host: bool = False) -> dict:
    """cslam::SearchByBoWBatch: SearchByBoW(key1, keys2[j]) for every candidate from ONE device call (host=True or a host-only store: the host evaluation).
    nmatches[C], matches12[C] (each one entry per feature of key1: the feature of keys2[j] or -1), reevaluated, and the table / counters of the one evaluation"""
    keys2 = np.ascontiguousarray(np.asarray(list(keys2), np.int64).reshape(-1))
    Cn = int(keys2.size)
    l1 = np.ascontiguousarray(np.asarray(live1, np.uint8).reshape(-1))
    off2, m2 = pack_masks(live2)
    h = _host().ccmh_bow_batch_create(store.handle, -1 if host else store.device, int(key1), Cn, _p(keys2), _p(l1), _p(off2), _p(m2), C.c_float(nnratio),
                                      int(bool(check_orientation)))
    if not h:
        raise CcmError("ccmh_bow_batch_create failed (bad arguments, a key that is not live or has no feature vector, or a device error)")
    try:
        N1 = int(l1.size)
        nm, m12 = [], []
        for j in range(Cn):
            m = np.zeros(N1, np.int32)
            n = _host().ccmh_bow_batch_result(h, j, N1, _p(m))
            if n < 0:
                raise CcmError(f"ccmh_bow_batch_result: {n}")
            nm.append(n); m12.append(m)
        table = np.zeros(N1 * Cn, np.uint64); nq = np.zeros(Cn, np.int32); nd = np.zeros(Cn, np.int32)
        _host().ccmh_bow_batch_table(h, _p(table), _p(nq), _p(nd))
        return dict(nmatches=nm, matches12=m12, reevaluated=int(_host().ccmh_bow_batch_n_reeval(h)), table=table, n_query=nq, n_dist=nd)
    finally:
        _host().ccmh_bow_batch_destroy(h)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# generator (numpy only; nothing here touches the device)
# ---------------------------------------------------------------------------------------------------------------------------------------------
PROFILE_SIZES = {"8x1000": dict(candidates=8, features=1000), "3x2000": dict(candidates=3, features=2000), "1x1000": dict(candidates=1, features=1000)}


def profile_scene(candidates: int, features: int, n_nodes: int = 80, seed: int = 0, live_share: float = 0.8) -> dict:
    """A place-recognition event: one current keyframe of `features` features over n_nodes vocabulary nodes and `candidates` keyframes that see the same scene
    (descriptors with 6 % of the bits flipped, shuffled; nine words in ten fall into the same node, 3 % are stopped).  Per keyframe: desc (n, 32), angle, the flat
    feature vector fv = (node, off, idx) and the live mask.  kfs[0] is the current keyframe."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (features, 32), dtype=np.uint8)
    node0 = rng.integers(0, n_nodes, features)
    ang0 = rng.uniform(0, 360, features).astype(np.float32)

    def fv_of(node_of):
        nodes = np.unique(node_of[node_of >= 0])
        order = np.argsort(node_of, kind="stable")
        order = order[node_of[order] >= 0]
        off = np.concatenate([[0], np.cumsum([(node_of == nd).sum() for nd in nodes])])
        return nodes.astype(np.int32), off.astype(np.int32), order.astype(np.int32)

    def view(k):
        perm = rng.permutation(features) if k else np.arange(features)
        bits = np.unpackbits(base[perm], axis=1)
        desc = np.packbits(bits ^ (rng.random(bits.shape) < (0.06 if k else 0.0)), axis=1)
        node = node0[perm].copy()
        moved = rng.random(features) < (0.1 if k else 0.0)
        node[moved] = rng.integers(0, n_nodes, int(moved.sum()))
        node[rng.random(features) < 0.03] = -1
        angle = (ang0[perm] + rng.normal(0, 2.0, features).astype(np.float32)) % np.float32(360.0)
        return dict(desc=np.ascontiguousarray(desc), angle=angle.astype(np.float32), fv=fv_of(node), live=(rng.random(features) < live_share).astype(np.uint8))
    return dict(kfs=[view(k) for k in range(candidates + 1)], n_nodes=n_nodes)
