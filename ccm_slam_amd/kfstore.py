"""The keyframe feature store (ccm_kfstore_* of the C ABI, cslam::KeyFrameStore of the host mirror): what ORBmatcher::Fuse reads of a keyframe and
no Fuse call changes — the 10-float record, mvKeysUn, the octaves, the descriptors and mGrid — uploaded once and kept on the device, and the two batched Fuse
stages on keyframes of the store.

KeyFrameStore(ctx, max_kf, max_feat) wraps cslam::KeyFrameStore, which keeps the device handle and a host shadow per live key; ctx = None asks for the host-only
store by name.  fuse_sim3_eval_resident / fuse_pose_eval_resident run ccm_fuse_sim3_eval_resident / ccm_fuse_pose_eval_resident and return the dictionaries of
fuse_sim3.fuse_sim3_eval / fuse_pose.fuse_pose_eval; the *_host forms evaluate the same pairs on the store's shadows through csrc/fuse_math.h.
SearchAndFuseBatchResident / SearchInNeighborsBatchResident are the mirrors' constructors on keys of a store.  set_featvec gives a key its feature vector, which
ComputeSim3's SearchByBoW reads (bow_search.py).  ingest brings the keyframes of a message into the store in one call: add without a grid, the
vocabulary transform and set_featvec for all of them, BowVector and FeatureVector returned (ccm_kfstore_ingest).

build_grid_keyframe replays KeyFrame::AssignFeaturesToGrid and KeyFrame::PosInGrid (cslam/src/KeyFrame.cpp:206-225, :265-275) line by line in Python; it shares
nothing with csrc/kfstore_math.h, which is what the tests compare it with.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Optional

import numpy as np

from . import fuse_pose as fp, fuse_sim3 as fs
from ._lib import CcmError, Context, _p, check, host, lib
from .fuse_sim3 import CELLS, GRID_COLS, GRID_ROWS, _c

E_ARG, E_STATE = -1, -6
KFI_MAX_FEAT = 4096   # csrc/kfingest_math.h: the most features of one keyframe of an ingest call


class StoreError(CcmError):
    """a refusal of the store; code = CCM_E_ARG (-1) or CCM_E_STATE (-6)"""

    def __init__(self, what: str, code: int):
        super().__init__(f"{what}: {code}")
        self.code = code


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    V, I, F = C.c_void_p, C.c_int, C.c_float
    h.ccmh_kfstore_create.restype = V
    h.ccmh_kfstore_create.argtypes = [I, I, I]
    h.ccmh_kfstore_destroy.restype = None
    h.ccmh_kfstore_destroy.argtypes = [V]
    h.ccmh_kfstore_add.argtypes = [V, I, I] + [V] * 8
    h.ccmh_kfstore_erase.argtypes = [V, I, C.c_int64]
    h.ccmh_kfstore_clear.argtypes = [V, I]
    h.ccmh_kfstore_count.argtypes = [V, V, V]
    h.ccmh_kfstore_handle.restype = V
    h.ccmh_kfstore_handle.argtypes = [V]
    h.ccmh_kfstore_get.argtypes = [V, I, C.c_int64, V, V, V, V]
    h.ccmh_kfstore_set_featvec.argtypes = [V, I, C.c_int64, I, V, V, V, V]
    h.ccmh_kfstore_ingest.argtypes = [V, I, V, I, I] + [V] * 16
    h.ccmh_kfstore_ingest_host.argtypes = [V, I, I] + [V] * 5 + [I, I] + [V] * 16
    h.ccmh_kfstore_shadow_equal.argtypes = [V, V, C.c_int64]      # a test aid: two stores' shadows of one key, field by field
    pts = [I] + [V] * 5
    h.ccmh_fuse_sim3_eval_resident_host.argtypes = [V, I, V, V, I, V, F, F] + pts + [V] * 4
    h.ccmh_fuse_pose_eval_resident_host.argtypes = [V, I, V, V, I, V, V, F, F] + pts + [I, V, V, V] + [V] * 4
    h.ccmh_fuse_sim3_create_resident.restype = V
    h.ccmh_fuse_sim3_create_resident.argtypes = [V, I, I, V, V, I, V, F, F] + pts
    h.ccmh_fuse_pose_create_resident.restype = V
    h.ccmh_fuse_pose_create_resident.argtypes = [V, I, I, V, V, I, V, V, F, F] + pts + [I, V, I, I]
    return h


@functools.lru_cache(maxsize=None)
def _dev():
    l = lib()
    V, I, F = C.c_void_p, C.c_int, C.c_float
    pts = [I] + [V] * 5
    l.ccm_fuse_sim3_eval_resident.argtypes = [V, V, I, V, V, I, V, F, F] + pts + [V] * 4
    l.ccm_fuse_pose_eval_resident.argtypes = [V, V, I, V, V, I, V, V, F, F] + pts + [I, V, V, V] + [V] * 4
    l.ccm_kfstore_ingest.argtypes = [V, V, V, I, I] + [V] * 15
    return l


def _round_half_away(t: np.float32) -> int:
    """round(float) of the C library for a finite t"""
    t = float(t)
    return int(math.floor(t + 0.5)) if t >= 0 else int(math.ceil(t - 0.5))


def build_grid_keyframe(xy, rec):
    """(cell_off[3601], cell_idx[n_in]) of a keyframe by ITS OWN rule: a literal replay of KeyFrame::AssignFeaturesToGrid (KeyFrame.cpp:206-225) with
    KeyFrame::PosInGrid (:265-275).  rec[4], rec[5] = mnMinX, mnMinY (ints), rec[8], rec[9] = mfGridElementWidthInv, mfGridElementHeightInv.  np.float32 arithmetic
    (one difference, one product), round half away from zero, a keypoint outside the grid in no cell, push_back order inside a cell.  A product no int holds (NaN,
    Inf) is stated as outside, as csrc/kfstore_math.h states it."""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    rec = np.asarray(rec, np.float32)
    mnMinX, mnMinY = np.float32(int(rec[4])), np.float32(int(rec[5]))
    wInv, hInv = np.float32(rec[8]), np.float32(rec[9])
    grid = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]      # mGrid[i][j]
    with np.errstate(all="ignore"):
        for i in range(xy.shape[0]):
            tx = np.float32(np.float32(xy[i, 0] - mnMinX) * wInv)
            ty = np.float32(np.float32(xy[i, 1] - mnMinY) * hInv)
            if not (np.isfinite(tx) and np.isfinite(ty)) or abs(float(tx)) >= 2.0 ** 31 or abs(float(ty)) >= 2.0 ** 31:
                continue
            posX, posY = _round_half_away(tx), _round_half_away(ty)
            if posX < 0 or posX >= GRID_COLS or posY < 0 or posY >= GRID_ROWS:
                continue
            grid[posX][posY].append(i)
    off = np.zeros(CELLS + 1, np.int32)
    idx = []
    for ix in range(GRID_COLS):
        for iy in range(GRID_ROWS):
            idx += grid[ix][iy]
            off[ix * GRID_ROWS + iy + 1] = len(idx)
    return off, np.array(idx, np.int32)


def _keys(keys) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(list(keys) if not isinstance(keys, np.ndarray) else keys, np.int64).reshape(-1))


def ingest_outputs(M: int, F: int, want_feat: bool = False):
    """ccm_kfstore_ingest's nine output arrays (the last two None unless asked for), every one with room for one element more than the call writes"""
    i32 = lambda n: np.zeros(n + 1, np.int32)
    return [i32(M), i32(F), np.zeros(F + 1, np.float64), i32(M), i32(F), i32(F + M), i32(F), i32(F) if want_feat else None, i32(F) if want_feat else None]


def tree_args(vocab):
    """the flat tree of ccm_vocab_create from a matcher.Vocabulary or a vocabulary dictionary: (n_nodes, L and the five arrays' pointers, the arrays themselves,
    which the caller holds for the length of the call)"""
    if isinstance(vocab, dict):
        dts = dict(child_off=np.int32, child_id=np.int32, node_desc=np.uint8, word_id=np.int32, weight=np.float64)
        keep = {k: np.ascontiguousarray(vocab[k], dt) for k, dt in dts.items()}
        n_nodes, L = int(vocab["n_nodes"]), int(vocab["L"])
    else:
        keep, n_nodes, L = vocab._keep, vocab.n_nodes, vocab.L
    return [n_nodes, L] + [_p(keep[k]) for k in ("child_off", "child_id", "node_desc", "word_id", "weight")], keep


def split_ingest(feat_off, out) -> list:
    """ccm_kfstore_ingest's flat outputs as one dictionary per keyframe"""
    bow_n, bow_word, bow_value, fv_nn, fv_node, fv_off, fv_idx, feat_word, feat_node = out
    res = []
    for m in range(bow_n.size - 1):
        f0, f1 = int(feat_off[m]), int(feat_off[m + 1])
        nw, nn = int(bow_n[m]), int(fv_nn[m])
        off = fv_off[f0 + m:f0 + m + nn + 1].copy()
        d = dict(bow_word=bow_word[f0:f0 + nw].copy(), bow_value=bow_value[f0:f0 + nw].copy(), fv_node=fv_node[f0:f0 + nn].copy(), fv_off=off,
                 fv_idx=fv_idx[f0:f0 + int(off[-1])].copy())
        if feat_word is not None:
            d.update(feat_word=feat_word[f0:f1].copy(), feat_node=feat_node[f0:f1].copy())
        res.append(d)
    return res


class KeyFrameStore:
    """cslam::KeyFrameStore.  ctx = None: the host-only store.  With a context the calls run on the calling thread's own context of ctx's device."""

    def __init__(self, ctx: Optional[Context], max_kf: int, max_feat: int):
        self.device = -1 if ctx is None else int(ctx.device)
        self._h = _host().ccmh_kfstore_create(self.device, int(max_kf), int(max_feat))
        if not self._h:
            raise CcmError("ccmh_kfstore_create failed (bad capacity or a device error)")
        if ctx is not None:
            ctx.adopt(self)

    @property
    def handle(self):
        return self._h

    @property
    def raw(self):
        """the ccm_kfstore* of include/ccm_hip.h (None for the host-only store)"""
        return _host().ccmh_kfstore_handle(self._h)

    def add(self, keys, rec, feat_off, feat_xy, feat_octave, feat_desc, cell_off=None, cell_idx=None):
        """M keyframes in one call, arrays as fuse_sim3.Scene holds them; without cell_off / cell_idx the store builds the grid by the keyframe's own rule"""
        keys = _keys(keys)
        a = [_c(rec, np.float32), _c(feat_off, np.int32), _c(feat_xy, np.float32), _c(feat_octave, np.uint8), _c(feat_desc, np.uint8), _c(cell_off, np.int32),
             _c(cell_idx, np.int32)]
        rc = _host().ccmh_kfstore_add(self._h, self.device, int(keys.size), _p(keys), *[_p(x) for x in a])
        if rc != 0:
            raise StoreError("ccmh_kfstore_add", rc)

    def add_scene(self, keys, s, kfs=None, grid: bool = False):
        """the keyframes `kfs` (default: all) of a fuse_sim3 / fuse_pose Scene under `keys`; grid: supply the scene's own grid instead of having it built"""
        kfs = list(range(s.K)) if kfs is None else list(kfs)
        sub = s.subset(kfs) if isinstance(s, fs.Scene) else s.subset(kfs, jobs=())
        self.add(keys, sub.rec, sub.feat_off, sub.feat_xy, sub.feat_octave, sub.feat_desc, sub.cell_off if grid else None, sub.cell_idx if grid else None)

    def set_featvec(self, key: int, fv, angle=None):
        """the key's DBoW2::FeatureVector as fv = (node[nn], off[nn + 1], idx[off[nn]]) (None: nn = 0) and mvKeysUn[i].angle (the shadow's alone; default zeros);
        fv = (nn, node, off, idx) passes raw arguments, None standing for a null pointer"""
        if fv is not None and len(fv) == 4:
            nn, node, off, idx = fv
            node, off, idx = (None if x is None else np.ascontiguousarray(x, np.int32) for x in (node, off, idx))
        else:
            node, off, idx = (np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32)) if fv is None else (np.ascontiguousarray(x, np.int32) for x in fv)
            nn = int(node.size)
        ang = None if angle is None else np.ascontiguousarray(angle, np.float32)
        rc = _host().ccmh_kfstore_set_featvec(self._h, self.device, int(key), int(nn), _p(node), _p(off), _p(idx), _p(ang))
        if rc != 0:
            raise StoreError("ccmh_kfstore_set_featvec", rc)

    def ingest(self, vocab, keys, rec, feat_off, feat_xy, feat_octave, feat_desc, angle=None, levelsup: int = 4, want_feat: bool = False):
        """The M keyframes of a message in ONE call (ccm_kfstore_ingest): add without a grid, the vocabulary transform and set_featvec for all of
        them.  vocab: a matcher.Vocabulary (device store) or, for the host-only store, that or the vocabulary dictionary of synth.make_vocabulary.  Returns one
        dictionary per keyframe: bow_word / bow_value (mBowVec: ascending word ids, L1-normalised) and fv_node / fv_off / fv_idx (mFeatVec, set_featvec's form);
        with want_feat also feat_word / feat_node, the descent's result per feature."""
        keys = _keys(keys)
        M = int(keys.size)
        rec, feat_off, feat_xy = _c(rec, np.float32), _c(feat_off, np.int32), _c(feat_xy, np.float32)
        feat_octave, feat_desc = _c(feat_octave, np.uint8), _c(feat_desc, np.uint8)
        ang = None if angle is None else np.ascontiguousarray(angle, np.float32)
        F = int(feat_off[M]) if M > 0 and feat_off is not None and feat_off.size > M else 0
        F = max(F, 0)
        out = ingest_outputs(M, F, want_feat)
        args = [int(levelsup), M, _p(keys), _p(rec), _p(feat_off), _p(feat_xy), _p(feat_octave), _p(feat_desc), _p(ang)] + [_p(x) for x in out]
        if self.device >= 0:
            if isinstance(vocab, dict):
                raise CcmError("KeyFrameStore.ingest: a device store needs a matcher.Vocabulary")
            rc = _host().ccmh_kfstore_ingest(self._h, self.device, vocab._h, *args)
        else:
            tree, _alive = tree_args(vocab)
            rc = _host().ccmh_kfstore_ingest_host(self._h, *tree, *args)
        if rc != 0:
            raise StoreError("ccmh_kfstore_ingest", rc)
        return split_ingest(feat_off, out)

    def erase(self, key: int):
        if _host().ccmh_kfstore_erase(self._h, self.device, int(key)) != 0:
            raise CcmError("ccmh_kfstore_erase failed")

    def clear(self):
        if _host().ccmh_kfstore_clear(self._h, self.device) != 0:
            raise CcmError("ccmh_kfstore_clear failed")

    def count(self):
        """(live keys, free slots)"""
        a, b = C.c_int(), C.c_int()
        _host().ccmh_kfstore_count(self._h, C.byref(a), C.byref(b))
        return a.value, b.value

    def get(self, key: int, shadow: bool = False) -> dict:
        """n, n_in, cell_off[3601], cell_idx[n_in] of one key: what the device holds, or (host-only store, or shadow=True) the host shadow"""
        n, n_in = C.c_int(), C.c_int()
        dev = -1 if shadow else self.device
        rc = _host().ccmh_kfstore_get(self._h, dev, int(key), C.byref(n), C.byref(n_in), None, None)
        if rc != 0:
            raise StoreError("ccmh_kfstore_get", rc)
        off = np.zeros(CELLS + 1, np.int32); idx = np.zeros(max(n.value, 1), np.int32)
        rc = _host().ccmh_kfstore_get(self._h, dev, int(key), C.byref(n), C.byref(n_in), _p(off), _p(idx))
        if rc != 0:
            raise StoreError("ccmh_kfstore_get", rc)
        return dict(n=n.value, n_in=n_in.value, cell_off=off, cell_idx=idx[:n_in.value].copy())

    def close(self):
        if self._h:
            _host().ccmh_kfstore_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _sim3_args(keys, s: fs.Scene):
    keys = _keys(keys)
    if s.Scw.size != 12 * keys.size:
        raise ValueError("one Scw per key")
    return keys, [int(keys.size), _p(keys), _p(s.Scw), s.nlevels, _p(s.scale_factors), C.c_float(s.log_sf), C.c_float(s.th), s.P, _p(s.pos), _p(s.normal),
                  _p(s.min_dist), _p(s.max_dist), _p(s.pt_desc)]


def _pose_args(keys, s: fp.Scene):
    keys = _keys(keys)
    if s.pose.size != 15 * keys.size:
        raise ValueError("one pose per key")
    return keys, [int(keys.size), _p(keys), _p(s.pose), s.nlevels, _p(s.scale_factors), _p(s.inv_sigma2), C.c_float(s.log_sf), C.c_float(s.th), s.P, _p(s.pos),
                  _p(s.normal), _p(s.min_dist), _p(s.max_dist), _p(s.pt_desc)]


class _Shape:
    """K and P as fuse_sim3._outputs / _result read them"""

    def __init__(self, K, P):
        self.K, self.P = K, P


def fuse_sim3_eval_resident(ctx: Context, store: KeyFrameStore, keys, s: fs.Scene, want_uv: bool = False) -> dict:
    """ccm_fuse_sim3_eval_resident on the live keys `keys` with the Scw, the level table and the points of `s` (whose own keyframe arrays are not read)"""
    keys, args = _sim3_args(keys, s)
    sh = _Shape(int(keys.size), s.P)
    table, nv, nh, uv = fs._outputs(sh, want_uv)
    check(_dev().ccm_fuse_sim3_eval_resident(ctx.handle, store.raw, *args, _p(table), _p(nv), _p(nh), _p(uv)), ctx.handle)
    return fs._result(sh, table, nv, nh, uv)


def fuse_sim3_eval_resident_host(store: KeyFrameStore, keys, s: fs.Scene, want_uv: bool = False) -> dict:
    keys, args = _sim3_args(keys, s)
    sh = _Shape(int(keys.size), s.P)
    table, nv, nh, uv = fs._outputs(sh, want_uv)
    if _host().ccmh_fuse_sim3_eval_resident_host(store.handle, *args, _p(table), _p(nv), _p(nh), _p(uv)) != 0:
        raise CcmError("ccmh_fuse_sim3_eval_resident_host: bad arguments or a key that is not live")
    return fs._result(sh, table, nv, nh, uv)


def fuse_pose_eval_resident(ctx: Context, store: KeyFrameStore, keys, s: fp.Scene, want_uv: bool = False) -> dict:
    """ccm_fuse_pose_eval_resident on the live keys `keys` with the poses, the level tables, the points and the jobs of `s` (job_kf indexes `keys`)"""
    keys, args = _pose_args(keys, s)
    table, nv, nh, uv = fp._outputs(s, want_uv)
    check(_dev().ccm_fuse_pose_eval_resident(ctx.handle, store.raw, *args, *s.job_args(), _p(table), _p(nv), _p(nh), _p(uv)), ctx.handle)
    return fp._result(s, table, nv, nh, uv)


def fuse_pose_eval_resident_host(store: KeyFrameStore, keys, s: fp.Scene, want_uv: bool = False) -> dict:
    keys, args = _pose_args(keys, s)
    table, nv, nh, uv = fp._outputs(s, want_uv)
    if _host().ccmh_fuse_pose_eval_resident_host(store.handle, *args, *s.job_args(), _p(table), _p(nv), _p(nh), _p(uv)) != 0:
        raise CcmError("ccmh_fuse_pose_eval_resident_host: bad arguments or a key that is not live")
    return fp._result(s, table, nv, nh, uv)


class SearchAndFuseBatchResident(fs.SearchAndFuseBatch):
    """cslam::SearchAndFuseBatch on keys of a store: ONE resident call at construction (the host evaluation for a host-only store), then resolve(k, ...)"""

    def __init__(self, store: KeyFrameStore, keys, s: fs.Scene):
        keys, args = _sim3_args(keys, s)
        self.scene = _Shape(int(keys.size), s.P)
        self._h = _host().ccmh_fuse_sim3_create_resident(store.handle, store.device, *args)
        if not self._h:
            raise CcmError("ccmh_fuse_sim3_create_resident failed (bad arguments, a key that is not live or a device error)")


class SearchInNeighborsBatchResident(fp.SearchInNeighborsBatch):
    """cslam::SearchInNeighborsBatch on keys of a store; targets and current index `keys`"""

    def __init__(self, store: KeyFrameStore, keys, s: fp.Scene, targets, current: Optional[int], n_current: int):
        keys, args = _pose_args(keys, s)
        self.scene = s
        self.targets = np.ascontiguousarray(targets, np.int32)
        self.C = int(self.targets.size); self.P1 = int(n_current); self.P2 = s.P - int(n_current)
        self.J = self.C + (current is not None)
        self._h = _host().ccmh_fuse_pose_create_resident(store.handle, store.device, *args, self.C, _p(self.targets), -1 if current is None else int(current), self.P1)
        if not self._h:
            raise CcmError("ccmh_fuse_pose_create_resident failed (bad arguments, a key that is not live or a device error)")
