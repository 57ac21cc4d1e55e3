"""Relocalisation behind the PnP pose: the guided search ORBmatcher::SearchByProjection(Frame&, kfptr, sAlreadyFound, th, ORBdist)
(cslam/src/ORBmatcher.cpp:1478-1604) and the refine chain that consumes one pose of pnp.PnPRansac.next().

guided_search runs ccm_frame_guided_search on a frame.FrameGrid: for all slots of the candidate keyframe the gates, the windows and the Hamming distances in one
call; guided_search_host runs the same lines (csrc/guided_search_math.h) with a host grid on the calling thread and touches no device.
search_by_projection_kf / _host are the mirror's two overloads (libccm_host.so): the evaluation followed by the sequential pass, and refine is
cslam::RelocalizationRefine.  A frame is (kps, desc): undistorted keypoints in the ccm_keypoint layout (frame.FrameGrid.set_keypoints) and N x 32 descriptor bytes.
"""
from __future__ import annotations

import ctypes as C
import functools
from dataclasses import dataclass

import numpy as np

from ._lib import CcmError, Context, _p, check, host, lib

SKIPPED, OUTSIDE, RANGE, SEARCHED = 0, 1, 2, 3
MAX_LEVELS = 16


class GuidedPose(C.Structure):
    """ccm_guided_pose"""
    _fields_ = [("Tcw", C.c_float * 12), ("logScaleFactor", C.c_float), ("nScaleLevels", C.c_int32), ("scaleFactors", C.c_float * 16)]


def guided_pose(Tcw, log_scale_factor, scale_factors, n_levels=None) -> GuidedPose:
    """Tcw: the frame's pose, 3x4 or 4x4 (rows 0..2 are used); scale_factors: mvScaleFactors"""
    T = np.asarray(Tcw, np.float32).reshape(-1)[:12]
    sf = np.asarray(scale_factors, np.float32).reshape(-1)
    p = GuidedPose()
    p.Tcw[:] = [float(x) for x in T]
    p.logScaleFactor = float(np.float32(log_scale_factor))
    p.nScaleLevels = int(sf.size if n_levels is None else n_levels)
    for i in range(min(sf.size, MAX_LEVELS)):
        p.scaleFactors[i] = float(sf[i])
    return p


@dataclass
class KeyFramePoints:
    """What the search reads from the candidate keyframe, per feature slot"""
    live: np.ndarray       # pMP && !pMP->isBad()
    pos: np.ndarray        # (n, 3) f32
    min_dist: np.ndarray
    max_dist: np.ndarray
    desc: np.ndarray       # (n, 32) u8
    angle: np.ndarray      # pKF->mvKeysUn[i].angle

    def __post_init__(self):
        self.live = np.ascontiguousarray(self.live, np.uint8)
        self.pos = np.ascontiguousarray(self.pos, np.float32).reshape(-1, 3)
        self.min_dist = np.ascontiguousarray(self.min_dist, np.float32)
        self.max_dist = np.ascontiguousarray(self.max_dist, np.float32)
        self.desc = np.ascontiguousarray(self.desc, np.uint8).reshape(-1, 32)
        self.angle = np.ascontiguousarray(self.angle, np.float32)

    @property
    def n(self) -> int:
        return int(self.live.size)


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    vp = C.c_void_p
    h.ccmh_guided_search_host.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 5 + [C.c_float] + [vp] * 7 + [C.c_int64, vp]
    h.ccmh_search_by_projection_kf_host.argtypes = [vp, vp, C.c_int, vp, vp, vp, C.c_int] + [vp] * 7 + [C.c_float, C.c_int, C.c_int, vp]
    h.ccmh_search_by_projection_kf_dev.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int] + [vp] * 7 + [C.c_float, C.c_int, C.c_int, vp]
    h.ccmh_search_by_projection_kf_cand.argtypes = [C.c_int, vp, vp, C.c_int, C.c_int] + [vp] * 4 + [C.c_int, C.c_int, vp]
    h.ccmh_reloc_refine.argtypes = [C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int] + [vp] * 12
    return h


def _frame(kps, desc):
    kps = np.ascontiguousarray(kps)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    assert kps.dtype.itemsize == 24 and kps.shape[0] == desc.shape[0]
    return kps, desc


def _points(pos, min_dist, max_dist, desc, skip):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    P = int(pos.shape[0])
    min_dist, max_dist = np.ascontiguousarray(min_dist, np.float32), np.ascontiguousarray(max_dist, np.float32)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    skip = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    assert min_dist.size == P and max_dist.size == P and desc.shape[0] == P and (skip is None or skip.size == P)
    return P, pos, min_dist, max_dist, desc, skip


def _guided(call, P, cap, what):
    """the capacity contract of ccm_frame_window_search; without a capacity of the caller's: one call with a typical one, one retry with the exact size"""
    retry = cap is None
    m = max(P, 1)
    status, u, v, level = np.zeros(m, np.uint8), np.zeros(m, np.float32), np.zeros(m, np.float32), np.zeros(m, np.int32)
    off = np.zeros(P + 1, np.int32)
    n = C.c_int64(0)
    cap = 24 * P + 1024 if cap is None else int(cap)
    idx, dist = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.uint16)
    rc = call(status, u, v, level, off, idx, dist, cap, n)
    if retry and rc != 0 and n.value > cap:
        cap = n.value
        idx, dist = np.zeros(cap, np.int32), np.zeros(cap, np.uint16)
        rc = call(status, u, v, level, off, idx, dist, cap, n)
    what(rc, n.value)
    k = n.value if cap else 0
    return dict(status=status[:P], u=u[:P], v=v[:P], level=level[:P], off=off, idx=idx[:k], dist=dist[:k], n_cand=n.value)


def guided_search(grid, pose: GuidedPose, pos, min_dist, max_dist, desc, skip=None, th: float = 10.0, cap=None):
    """ccm_frame_guided_search on a frame.FrameGrid.  Returns dict(status, u, v, level, off, idx, dist, n_cand); cap = 0 is the sizing call (no idx / dist)."""
    P, pos, min_dist, max_dist, desc, skip = _points(pos, min_dist, max_dist, desc, skip)

    def call(status, u, v, level, off, idx, dist, cap, n):
        return lib().ccm_frame_guided_search(grid._h, C.byref(pose), P, _p(pos), _p(min_dist), _p(max_dist), _p(desc), _p(skip), C.c_float(th), _p(status), _p(u), _p(v),
                                             _p(level), _p(off), _p(idx), _p(dist), C.c_int64(cap), C.byref(n))

    def what(rc, n_cand):
        try:
            check(rc, grid.ctx.handle)
        except CcmError as e:
            e.rc, e.n_cand = rc, n_cand        # a capacity that is too small: CCM_E_ARG with the number of candidates
            raise
    return _guided(call, P, cap, what)


def guided_search_host(kps, fdesc, bounds, K, pose: GuidedPose, pos, min_dist, max_dist, desc, skip=None, th: float = 10.0, cap=None):
    """The host evaluator of ccm_frame_guided_search (no device).  bounds = mnMinX mnMinY mnMaxX mnMaxY, K = fx fy cx cy."""
    kps, fdesc = _frame(kps, fdesc)
    bounds, K = np.ascontiguousarray(bounds, np.float32), np.ascontiguousarray(K, np.float32)
    P, pos, min_dist, max_dist, desc, skip = _points(pos, min_dist, max_dist, desc, skip)

    def call(status, u, v, level, off, idx, dist, cap, n):
        return _host().ccmh_guided_search_host(_p(kps), _p(fdesc), int(kps.shape[0]), _p(bounds), _p(K), C.addressof(pose), P, _p(pos), _p(min_dist), _p(max_dist),
                                               _p(desc), _p(skip), C.c_float(th), _p(status), _p(u), _p(v), _p(level), _p(off), _p(idx), _p(dist), cap, C.addressof(n))

    def what(rc, n_cand):
        if rc:
            e = CcmError(f"ccmh_guided_search_host: {'bad arguments' if rc == -1 else rc}")
            e.rc, e.n_cand = rc, n_cand
            raise e
    return _guided(call, P, cap, what)


def _mp(frame_mp, N):
    mp = np.full(max(N, 1), -1, np.int32)
    if frame_mp is not None:
        mp[:N] = np.asarray(frame_mp, np.int32)
    return mp


def _rc(name, rc):
    if rc < 0:
        raise CcmError(f"{name}: {'bad arguments' if rc == -1 else 'the device path failed' if rc == -1000 else rc}")
    return rc


def search_by_projection_kf_host(kps, fdesc, bounds, K, pose: GuidedPose, kf: KeyFramePoints, already_found=None, th: float = 10.0, orb_dist: int = 100,
                                 check_orientation: bool = True, frame_mp=None):
    """The mirror's overload without a grid (no device).  Returns (nmatches, mvpMapPoints): a keyframe slot per frame feature, or -1."""
    kps, fdesc = _frame(kps, fdesc)
    N = int(kps.shape[0])
    bounds, K = np.ascontiguousarray(bounds, np.float32), np.ascontiguousarray(K, np.float32)
    found = None if already_found is None else np.ascontiguousarray(already_found, np.uint8)
    mp = _mp(frame_mp, N)
    rc = _host().ccmh_search_by_projection_kf_host(_p(kps), _p(fdesc), N, _p(bounds), _p(K), C.addressof(pose), kf.n, _p(kf.live), _p(kf.pos), _p(kf.min_dist),
                                                   _p(kf.max_dist), _p(kf.desc), _p(kf.angle), _p(found), C.c_float(th), int(orb_dist), int(bool(check_orientation)), _p(mp))
    return _rc("ccmh_search_by_projection_kf_host", rc), mp[:N]


def search_by_projection_kf(ctx: Context, K, width: int, height: int, kps, fdesc, pose: GuidedPose, kf: KeyFramePoints, already_found=None, th: float = 10.0,
                            orb_dist: int = 100, check_orientation: bool = True, frame_mp=None):
    """The mirror's overload with a grid: ONE ccm_frame_guided_search call, then the sequential pass.  Returns (nmatches, mvpMapPoints)."""
    kps, fdesc = _frame(kps, fdesc)
    N = int(kps.shape[0])
    K = np.ascontiguousarray(K, np.float32)
    found = None if already_found is None else np.ascontiguousarray(already_found, np.uint8)
    mp = _mp(frame_mp, N)
    rc = _host().ccmh_search_by_projection_kf_dev(ctx.device, _p(K), int(width), int(height), _p(kps), _p(fdesc), N, C.addressof(pose), kf.n, _p(kf.live), _p(kf.pos),
                                                  _p(kf.min_dist), _p(kf.max_dist), _p(kf.desc), _p(kf.angle), _p(found), C.c_float(th), int(orb_dist),
                                                  int(bool(check_orientation)), _p(mp))
    return _rc("ccmh_search_by_projection_kf_dev", rc), mp[:N]


def search_by_projection_kf_candidates(ctx: Context, fdesc, f_angle, desc, kf_angle, cand_off, cand_idx, orb_dist: int = 100, check_orientation: bool = True,
                                       frame_mp=None):
    """The drop-in's form (shim/ORBmatcher_hip.cpp): the gates and the window lists are the caller's (cand_off over the keyframe's slots, empty where a slot does not
    reach GetFeaturesInArea); ONE ccm_hamming_csr launch, then the sequential pass.  Returns (nmatches, mvpMapPoints)."""
    fdesc = np.ascontiguousarray(fdesc, np.uint8).reshape(-1, 32)
    N = int(fdesc.shape[0])
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    fa, ka = np.ascontiguousarray(f_angle, np.float32), np.ascontiguousarray(kf_angle, np.float32)
    off, idx = np.ascontiguousarray(cand_off, np.int32), np.ascontiguousarray(cand_idx, np.int32)
    assert fa.size == N and ka.size == desc.shape[0] and off.size == desc.shape[0] + 1
    if idx.size == 0:
        idx = np.zeros(1, np.int32)
    mp = _mp(frame_mp, N)
    rc = _host().ccmh_search_by_projection_kf_cand(ctx.device, _p(fdesc), _p(fa), N, int(desc.shape[0]), _p(desc), _p(ka), _p(off), _p(idx), int(orb_dist),
                                                   int(bool(check_orientation)), _p(mp))
    return _rc("ccmh_search_by_projection_kf_cand", rc), mp[:N]


@dataclass
class RefineResult:
    matched: bool
    n_good: int
    Tcw: np.ndarray        # (4, 4) f32, the frame's pose at the end
    map_points: np.ndarray  # mvpMapPoints: a keyframe slot per frame feature, or -1
    trace: np.ndarray      # nGood of optimisation 1, nadd of search 1, nGood 2, nadd 2, nGood 3; -1: the step did not run


def refine(ctx: Context, K, width: int, height: int, kps, fdesc, inv_level_sigma2, frame: GuidedPose, kf: KeyFramePoints, matches_f, inliers) -> RefineResult:
    """cslam::RelocalizationRefine: frame.Tcw is the pose pnp.PnPRansac.next() returned, matches_f the SearchByBoW(KF, F) table (a keyframe slot per frame feature
    or -1), inliers the pose's vbInliers."""
    kps, fdesc = _frame(kps, fdesc)
    N = int(kps.shape[0])
    K = np.ascontiguousarray(K, np.float32)
    isig = np.ascontiguousarray(inv_level_sigma2, np.float32)
    mf, inl = np.ascontiguousarray(matches_f, np.int32), np.ascontiguousarray(inliers, np.uint8)
    assert mf.size == N and inl.size == N
    mp = np.full(max(N, 1), -1, np.int32)
    T, trace, ngood = np.zeros(16, np.float32), np.zeros(5, np.int32), C.c_int32(0)
    rc = _host().ccmh_reloc_refine(ctx.device, _p(K), int(width), int(height), _p(kps), _p(fdesc), N, _p(isig), C.addressof(frame), kf.n, _p(kf.live), _p(kf.pos),
                                   _p(kf.min_dist), _p(kf.max_dist), _p(kf.desc), _p(kf.angle), _p(mf), _p(inl), _p(mp), _p(T), _p(trace), C.addressof(ngood))
    _rc("ccmh_reloc_refine", rc)
    return RefineResult(bool(rc), ngood.value, T.reshape(4, 4), mp[:N], trace)
