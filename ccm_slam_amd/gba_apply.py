"""A finished global BA applied to the map (Optimizer.cpp:803-857, then the walk of RunGBA: Map.cpp:1441-1568, LoopFinder.cpp ~895-1010, MapMerger.cpp ~640-755).

apply_map is ccm_gba_apply_map (include/ccm_hip.h): one packed copy in, at most three launches, one copy out; with `ba` it reads the optimised state from a BA
handle on the device instead of from host arrays.  apply_map_host runs the same lines compiled for the host (libccm_host.so).  MapUpdate is the host mirror
cslam::GbaMapUpdate: it takes the spanning tree as child sets and flattens it into the order of the reference's list walk.  make_scene generates seeded maps (a
forest over several origins; keyframes that were no vertices in chains, in a branching subtree and above a vertex; points of every kind) at the three sizes of
SIZES; flatten turns a scene into the flat arguments.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

import numpy as np

from ._lib import CcmError, Context, _arr, _p, check, host, lib
from .sim3_correct import _quat, _rot, camera_center

# keyframes of the walk, non-bad map points: a loop-sized map, one agent's map, the 4-agent map
SIZES = {"loop": (30, 3000), "agent": (500, 37500), "agents4": (2000, 150000)}
# the kinds of point the walk's second loop tells apart
PT_VERTEX, PT_MOVED, PT_NO_REF, PT_REF_UNTAGGED, PT_REF_UNREACHED = range(5)

# ccm_gba_apply_map after the context and before the handle / after it
_FLAT_IN = [C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
_FLAT_OUT = [C.c_void_p] * 4


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    h.ccmh_gbaupd_create.restype = C.c_void_p
    h.ccmh_gbaupd_create.argtypes = [C.c_int] * 3 + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    h.ccmh_gbaupd_sizes.argtypes = [C.c_void_p] * 2
    h.ccmh_gbaupd_results.argtypes = [C.c_void_p] * 7
    h.ccmh_gbaupd_destroy.argtypes = [C.c_void_p]
    h.ccmh_gbaupd_destroy.restype = None
    h.ccmh_gba_apply_map_host.argtypes = _FLAT_IN + _FLAT_OUT
    return h


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the flat call
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _flat_call(fn, first, f: dict, handle=()):
    """f: the keys of flatten.  `handle`: () or (ccm_ba*,), placed between the inputs and the outputs.  Returns (rc, outputs)."""
    par = _arr(f["kf_parent"], np.int32); cam = _arr(f["kf_cam"], np.int32)
    Tcw = _arr(f["Tcw_old"], np.float32); Twc = _arr(f["Twc_old"], np.float32)
    n_kf = int(f.get("n_kf", par.size if par is not None else 0))
    pos = _arr(f.get("pos"), np.float32); vert = _arr(f.get("pt_vert"), np.int32); ref = _arr(f.get("pt_ref"), np.int32)
    n_pt = int(f.get("n_pt", 0 if pos is None else pos.size // 3))
    cq = _arr(f.get("cam_qt"), np.float64); px = _arr(f.get("pt_xyz"), np.float64)
    n_cam = int(f.get("n_cam", 0 if cq is None else cq.size // 7)); n_lm = int(f.get("n_lm", 0 if px is None else px.size // 3))
    T_new = np.zeros(12 * max(n_kf, 1), np.float32); Twc_new = np.zeros(12 * max(n_kf, 1), np.float32)
    pos_out = np.zeros(3 * max(n_pt, 1), np.float32); status = np.full(max(n_pt, 1), 255, np.uint8)
    outs = [None if f.get("null_" + k) else v for k, v in (("T_new", T_new), ("Twc_new", Twc_new), ("pos_out", pos_out), ("pt_status", status))]
    rc = fn(*first, n_kf, _p(par), _p(cam), _p(Tcw), _p(Twc), n_pt, _p(pos), _p(vert), _p(ref), n_cam, _p(cq), n_lm, _p(px), *handle, *(_p(o) for o in outs))
    return rc, dict(T_new=T_new[:12 * n_kf].reshape(-1, 12), Twc_new=Twc_new[:12 * n_kf].reshape(-1, 12), pos=pos_out[:3 * n_pt].reshape(-1, 3), status=status[:n_pt])


def apply_map(ctx: Context, flat: dict, ba=None) -> dict:
    """ccm_gba_apply_map on the arguments of flatten.  ba: a BAHandle (optimizer.py) whose device state is read; flat's cam_qt / pt_xyz must then be None."""
    fn = lib().ccm_gba_apply_map
    fn.argtypes = [C.c_void_p] + _FLAT_IN + [C.c_void_p] + _FLAT_OUT
    rc, out = _flat_call(fn, (ctx.handle,), flat, (ba._h if ba is not None else None,))
    check(rc, ctx.handle)
    return out


def apply_map_host(flat: dict) -> dict:
    """The same arguments (host form) through gba_apply_math.h compiled for the host, on the calling thread (ccmh_gba_apply_map_host)."""
    rc, out = _flat_call(_host().ccmh_gba_apply_map_host, (), flat)
    if rc != 0:
        raise CcmError(f"ccmh_gba_apply_map_host: bad arguments ({rc})")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the host mirror
# ---------------------------------------------------------------------------------------------------------------------------------------------
class MapUpdate:
    """cslam::GbaMapUpdate on a scene (the keys of make_scene).  device None: the host evaluator, asked for by name."""

    def __init__(self, sc: dict, device: Optional[int] = None):
        a = [_arr(sc[k], np.int32) for k in ("origins", "child_off", "child_kf", "kf_cam")] + [_arr(sc["Tcw"], np.float32), _arr(sc["Twc"], np.float32)]
        p = [_arr(sc["pos"], np.float32), _arr(sc["pt_vert"], np.int32), _arr(sc["pt_ref_kf"], np.int32)]
        cq = _arr(sc["cam_qt"], np.float64); px = _arr(sc["pt_xyz"], np.float64)
        self.n_pt = p[1].size
        h = _host().ccmh_gbaupd_create(-1 if device is None else int(device), a[3].size, a[0].size, *(_p(x) for x in a), self.n_pt, *(_p(x) for x in p), cq.size // 7,
                                       _p(cq), px.size // 3, _p(px))
        if not h:
            raise CcmError("ccmh_gbaupd_create: bad arguments or device error")
        self._h = C.c_void_p(h)
        s = np.zeros(4, np.int64)
        _host().ccmh_gbaupd_sizes(self._h, _p(s))
        self.n_reached, self.reached_twice, self.stale_references = int(s[0]), int(s[1]), int(s[2])

    def results(self) -> dict:
        k, n = self.n_reached, max(self.n_pt, 1)
        o = dict(order=np.zeros(k, np.int32), kf_parent=np.zeros(k, np.int32), T_new=np.zeros((k, 12), np.float32), Twc_new=np.zeros((k, 12), np.float32),
                 pos=np.zeros((n, 3), np.float32), status=np.zeros(n, np.uint8))
        _host().ccmh_gbaupd_results(self._h, *(_p(o[x]) for x in ("order", "kf_parent", "T_new", "Twc_new", "pos", "status")))
        o["pos"] = o["pos"][:self.n_pt]; o["status"] = o["status"][:self.n_pt]
        return o

    def close(self):
        if self._h:
            _host().ccmh_gbaupd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------
def inverse_pose(T):
    """rows 0..2 of the Twc that KeyFrame::SetPose leaves for poses (n, 12) f32: [Rcw' | Ow]"""
    T = np.asarray(T, np.float32).reshape(-1, 12)
    W = np.zeros_like(T)
    for r in range(3):
        W[:, 4 * r] = T[:, r]; W[:, 4 * r + 1] = T[:, 4 + r]; W[:, 4 * r + 2] = T[:, 8 + r]
    W[:, 3::4] = camera_center(T)
    return W


def make_scene(seed: int = 0, n_kf: int = 30, n_pt: int = 3000, n_origins: int = 2, chains=(1, 2, 5), branching: bool = True, vertex_below: bool = True,
               extra_nonvert: Optional[int] = None, n_unreached: int = 2, vertex_frac: float = 0.85, moved_frac: float = 0.09, wide_level: int = 0) -> dict:
    """A forest of n_kf keyframes over n_origins origins, every keyframe with a random id.  Most are vertices of the BA (kf_cam >= 0, cameras in random order, a
    few cameras of the problem unused); hanging below vertices: one chain of keyframes that were no vertices per entry of `chains` (its depth), a branching
    subtree of them (a root with three children, one of which has two), a vertex below one of them with another non-vertex below it, `extra_nonvert` single ones,
    and `wide_level` of them under ONE vertex parent.  n_unreached vertices and as many non-vertices hang in no child set (the walk does not reach them).  Child
    sets come in random order (the reference's std::set is ordered by pointer).  Points: vertex_frac landmarks of the BA, moved_frac that move with a reached
    reference keyframe (a vertex or not), the rest split between no reference, an untagged (non-vertex, unreached) and a tagged unreached (vertex) reference."""
    rng = np.random.default_rng(seed)
    parent, vertex = [], []   # by construction index; parent -2: unreached

    def add(p, v):
        parent.append(p); vertex.append(v)
        return len(parent) - 1

    special = sum(chains) + (6 if branching else 0) + (3 if vertex_below else 0) + wide_level
    if extra_nonvert is None:
        extra_nonvert = max(0, min(n_kf // 100, 8))
    n_vert_tree = n_kf - special - extra_nonvert - 2 * n_unreached
    if n_vert_tree < n_origins:
        raise ValueError("n_kf too small for the requested structure")
    for i in range(n_vert_tree):   # the vertices: mostly a chain per origin (the spanning tree follows the trajectory), some side branches
        add(-1 if i < n_origins else (int(rng.integers(0, i)) if rng.random() < 0.15 else max(0, i - n_origins)), True)
    pick = lambda: int(rng.integers(0, n_vert_tree))
    chain_ends = []
    for d in chains:
        k = pick()
        for _ in range(d):
            k = add(k, False)
        chain_ends.append(k)
    if branching:
        r = add(pick(), False)
        c = [add(r, False) for _ in range(3)]
        add(c[1], False); add(c[1], False)
    if vertex_below:
        a = add(pick(), False)
        b = add(a, True)
        add(b, False)
    for _ in range(extra_nonvert):
        add(pick(), False)
    wp = pick()
    for _ in range(wide_level):
        add(wp, False)
    unreached_v = [add(-2, True) for _ in range(n_unreached)]
    unreached_n = [add(-2, False) for _ in range(n_unreached)]
    n = len(parent)
    assert n == n_kf
    ident = rng.permutation(n).astype(np.int32)   # construction index -> keyframe id
    parent = np.asarray(parent); vertex = np.asarray(vertex)
    origins = ident[np.nonzero(parent == -1)[0]]
    # child sets in random order
    has_p = np.nonzero(parent >= 0)[0]
    has_p = has_p[rng.permutation(has_p.size)]
    pid = ident[parent[has_p]]
    so = np.argsort(pid, kind="stable")
    child_kf = ident[has_p[so]].astype(np.int32)
    child_off = np.concatenate([[0], np.cumsum(np.bincount(pid, minlength=n))]).astype(np.int32)
    # cameras: the vertices in random order among n_cam cameras
    n_v = int(vertex.sum()); n_cam = n_v + 3
    kf_cam = np.full(n, -1, np.int32)
    kf_cam[ident[np.nonzero(vertex)[0]]] = rng.permutation(n_cam)[:n_v]
    # poses before the walk and the optimised ones: a trajectory with drift taken out
    s = np.arange(n) * 0.3
    cen = np.stack([8 * np.sin(s / 8), 0.3 * np.sin(s / 3), 8 * (1 - np.cos(s / 8)) + 0.2 * s], 1) + rng.normal(0, 0.03, (n, 3))
    R = _rot(np.stack([rng.normal(0, 0.05, n), s / 8 + rng.normal(0, 0.05, n), rng.normal(0, 0.05, n)], 1))
    t = -(R @ cen[:, :, None])[:, :, 0]
    Tcw = np.zeros((n, 12), np.float32)
    Tcw[ident] = np.concatenate([R, t[:, :, None]], 2).reshape(n, 12).astype(np.float32)
    Twc = inverse_pose(Tcw)
    cam_qt = np.zeros((n_cam, 7)); cam_qt[:, 3] = 1.0
    dR = _rot(rng.normal(0, 0.02, (n, 3)))
    Rn = dR @ R; tn = (dR @ t[:, :, None])[:, :, 0] * 1.01 + rng.normal(0, 0.05, (n, 3))
    for i in np.nonzero(vertex)[0]:
        cam_qt[kf_cam[ident[i]]] = np.concatenate([_quat(Rn[i]) * (1 + 1e-9 * rng.normal()), tn[i]])   # g2o does not renormalise: neither does the recovery
    # points
    kind = np.full(n_pt, PT_VERTEX, np.int32)
    u = rng.random(n_pt)
    rest = (1 - vertex_frac - moved_frac) / 3
    kind[u >= vertex_frac] = PT_MOVED
    for j, kd in enumerate((PT_NO_REF, PT_REF_UNTAGGED, PT_REF_UNREACHED)):
        kind[u >= vertex_frac + moved_frac + j * rest] = kd
    if n_unreached == 0:
        kind[kind >= PT_REF_UNTAGGED] = PT_NO_REF
    for j, kd in enumerate((PT_VERTEX, PT_MOVED, PT_NO_REF) + ((PT_REF_UNTAGGED, PT_REF_UNREACHED) if n_unreached else ())):   # every kind is present
        if n_pt >= 5:
            kind[j] = kd
    reached = np.nonzero(parent > -2)[0]
    base = rng.integers(0, n, n_pt)
    pos = (cen[base] + rng.normal(0, 1.0, (n_pt, 3)) + (R[base].transpose(0, 2, 1) @ np.array([0, 0, 4.0]))).astype(np.float32)
    ref_c = reached[rng.integers(0, reached.size, n_pt)]
    nonv_reached = np.nonzero((parent > -2) & ~vertex)[0]
    if nonv_reached.size:   # a third of the moved points hang on keyframes that were no vertices
        m = (kind == PT_MOVED) & (rng.random(n_pt) < 0.34)
        ref_c[m] = nonv_reached[rng.integers(0, nonv_reached.size, int(m.sum()))]
    if n_unreached:
        m = kind == PT_REF_UNTAGGED; ref_c[m] = np.asarray(unreached_n)[rng.integers(0, n_unreached, int(m.sum()))]
        m = kind == PT_REF_UNREACHED; ref_c[m] = np.asarray(unreached_v)[rng.integers(0, n_unreached, int(m.sum()))]
    pt_ref_kf = np.where(kind == PT_NO_REF, -1, ident[ref_c]).astype(np.int32)
    n_lm = int((kind == PT_VERTEX).sum()) + 5
    pt_vert = np.full(n_pt, -1, np.int32)
    pt_vert[kind == PT_VERTEX] = rng.permutation(n_lm)[:n_lm - 5]
    pt_xyz = rng.normal(0, 5.0, (n_lm, 3))
    sel = kind == PT_VERTEX
    pt_xyz[pt_vert[sel]] = pos[sel].astype(np.float64) + rng.normal(0, 0.05, (int(sel.sum()), 3))
    # vertices keep their reference too: the reference never looks at it
    return dict(n_kf=n, origins=origins.astype(np.int32), child_off=child_off, child_kf=child_kf, kf_cam=kf_cam, Tcw=Tcw, Twc=Twc, cam_qt=cam_qt, pt_xyz=pt_xyz, pos=pos,
                pt_vert=pt_vert, pt_ref_kf=pt_ref_kf, pt_kind=kind, chain_ends=ident[np.asarray(chain_ends, np.int64)] if chain_ends else np.zeros(0, np.int32),
                unreached_vertex=ident[np.asarray(unreached_v, np.int64)] if n_unreached else np.zeros(0, np.int32))


def flatten(sc: dict) -> dict:
    """The arguments of apply_map / apply_map_host for a scene (what cslam::GbaMapUpdate builds): the keyframes in the order of the list walk.  `order`: keyframe
    id per walk position; n_twice: keyframes reached a second time (> 0: the flat form does not describe the reference's walk); n_stale: points without a
    landmark whose reference keyframe is a vertex that the walk did not reach (left untouched)."""
    off = np.asarray(sc["child_off"]); ch = np.asarray(sc["child_kf"]); n = int(sc["n_kf"])
    at = np.full(n, -1, np.int64)
    order, par, n_twice = [], [], 0
    for o in sc["origins"]:
        if at[o] >= 0:
            n_twice += 1; continue
        at[o] = len(order); order.append(int(o)); par.append(-1)
    head = 0
    while head < len(order):
        k = order[head]
        for c in ch[off[k]:off[k + 1]]:
            if at[c] >= 0:
                n_twice += 1; continue
            at[c] = len(order); order.append(int(c)); par.append(head)
        head += 1
    order = np.asarray(order, np.int32)
    ref = np.asarray(sc["pt_ref_kf"])
    pt_ref = np.where(ref >= 0, at[np.maximum(ref, 0)], -1).astype(np.int32)
    stale = (ref >= 0) & (pt_ref < 0) & (np.asarray(sc["kf_cam"])[np.maximum(ref, 0)] >= 0) & (np.asarray(sc["pt_vert"]) < 0)
    return dict(n_kf=order.size, order=order, kf_parent=np.asarray(par, np.int32), kf_cam=np.asarray(sc["kf_cam"], np.int32)[order],
                Tcw_old=np.asarray(sc["Tcw"], np.float32).reshape(-1, 12)[order], Twc_old=np.asarray(sc["Twc"], np.float32).reshape(-1, 12)[order],
                pos=np.asarray(sc["pos"], np.float32), pt_vert=np.asarray(sc["pt_vert"], np.int32), pt_ref=pt_ref, cam_qt=np.asarray(sc["cam_qt"], np.float64),
                pt_xyz=np.asarray(sc["pt_xyz"], np.float64), n_twice=n_twice, n_stale=int(stale.sum()))
