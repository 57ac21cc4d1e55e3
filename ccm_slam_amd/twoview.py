"""Two-view (monocular) initialisation: the arithmetic of cslam::Initializer (cslam/src/Initializer.cpp) between the set drawing and the accept / reject
logic of ReconstructF / ReconstructH.

ransac_eval runs ccm_twoview_ransac_eval (the 2 x H eight-point models of FindHomography / FindFundamental, each scored against every match), check_rt runs
ccm_twoview_check_rt (every inlier under up to 8 motion hypotheses); ransac_eval_host / check_rt_host run the same lines compiled for the host
(libccm_host.so).  TwoViewInitializer is the host mirror cslam::TwoViewInitializer.  normalize, inv33, prepare_rt, svd and score_host expose single functions
of csrc/twoview_math.h as g++ compiles them.

The generators below make the planar and the general two-view scene of the tests: EuRoC intrinsics, 3 degrees of yaw, t = (-0.3, 0.02, 0.05), pixel noise.
They only produce numpy arrays.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional

import numpy as np

from . import synth
from ._lib import CcmError, Context, _p, check, hooks, host, lib

STATUS = ("not an inlier", "non-finite", "depth 1", "depth 2", "reprojection 1", "reprojection 2", "counted, low parallax", "good")
REC_FLOATS = 27


@functools.lru_cache(maxsize=None)
def _host():
    h = host()
    V = C.c_void_p
    h.ccmh_twoview_create.restype = V
    h.ccmh_twoview_create.argtypes = [C.c_int, V, C.c_int, V, C.c_float]
    h.ccmh_twoview_find.argtypes = [V, C.c_int, V, V, C.c_int] + [V] * 7
    h.ccmh_twoview_check_rt.argtypes = [V, C.c_int, V, V, C.c_float] + [V] * 5
    h.ccmh_twoview_destroy.argtypes = [V]
    h.ccmh_twoview_destroy.restype = None
    h.ccmh_twoview_draw_sets.argtypes = [C.c_int, C.c_int, V, V]
    h.ccmh_twoview_ransac_eval_host.argtypes = [C.c_int] + [V] * 7 + [C.c_float, C.c_int, V, C.c_int] + [V] * 6
    h.ccmh_twoview_check_rt_host.argtypes = [C.c_int, V, V, C.c_int, V, V, V, C.c_float, V, V, V]
    h.ccmh_twoview_normalize.argtypes = [V, C.c_int, V, V]
    h.ccmh_twoview_normalize.restype = None
    h.ccmh_twoview_inv33.argtypes = [V, V]
    h.ccmh_twoview_inv33.restype = None
    h.ccmh_twoview_prepare_rt.argtypes = [V] * 4
    h.ccmh_twoview_prepare_rt.restype = None
    h.ccmh_twoview_svd.argtypes = [C.c_int, V, V]
    h.ccmh_twoview_score_host.argtypes = [C.c_int, C.c_int, V, C.c_int, V, V, C.c_float, V, V]
    return h


def _f32(a, shape=(-1,)):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(shape))


def _i32(a, shape=(-1,)):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(shape))


def K_matrix(K=synth.EUROC_K) -> np.ndarray:
    """mK as a 3x3 f32"""
    fx, fy, cx, cy = K
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def mask_bits(mask, N: int) -> np.ndarray:
    """(..., ceil(N / 32)) words -> (..., N) booleans"""
    m = np.asarray(mask, np.uint32)
    bits = (m[..., :, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(m.shape[:-1] + (-1,))[..., :N].astype(bool)


def bits_mask(flags) -> np.ndarray:
    """N booleans -> ceil(N / 32) words"""
    f = np.asarray(flags, bool).reshape(-1)
    pad = np.zeros(((f.size + 31) // 32) * 32, np.uint32)
    pad[:f.size] = f
    return (pad.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(1).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# single functions of twoview_math.h, compiled for the host
# ---------------------------------------------------------------------------------------------------------------------------------------------
def normalize(xy):
    """Normalize (:745-791) over all keypoints of a frame: (pn (n, 2), T (3, 3))"""
    xy = _f32(xy, (-1, 2))
    pn = np.zeros_like(xy); T = np.zeros((3, 3), np.float32)
    _host().ccmh_twoview_normalize(_p(xy), int(len(xy)), _p(pn), _p(T))
    return pn, T


def inv33(S) -> np.ndarray:
    S = _f32(S); D = np.zeros(9, np.float32)
    _host().ccmh_twoview_inv33(_p(S), _p(D))
    return D.reshape(3, 3)


def prepare_rt(K, R, t) -> np.ndarray:
    """The 27-float record of one motion hypothesis: P2 = K [R | t], O2 = -R' t, R, t"""
    K = _f32(K); R = _f32(R); t = _f32(t); rec = np.zeros(REC_FLOATS, np.float32)
    _host().ccmh_twoview_prepare_rt(_p(K), _p(R), _p(t), _p(rec))
    return rec


def svd(A):
    """cv::SVDecomp(A, w, u, vt, MODIFY_A | FULL_UV) as restated, by shape: (16, 9) -> vt.row(8); (8, 9) -> vt (9, 9); (3, 3) -> (w, u, vt)"""
    A = np.asarray(A, np.float32)
    shape = {(16, 9): 0, (8, 9): 1, (3, 3): 2}[A.shape]
    out = np.zeros((9, 81, 21)[shape], np.float32)
    if _host().ccmh_twoview_svd(shape, _p(_f32(A)), _p(out)) != 0:
        raise CcmError("ccmh_twoview_svd: bad arguments")
    if shape == 0:
        return out
    if shape == 1:
        return out.reshape(9, 9)
    return out[:3].copy(), out[3:12].reshape(3, 3).copy(), out[12:].reshape(3, 3).copy()


def _score_args(model, M, xy1, xy2):
    M = _f32(M, (-1, 9)); xy1 = _f32(xy1, (-1, 2)); xy2 = _f32(xy2, (-1, 2))
    if model not in (0, 1) or len(M) < 1 or len(xy1) < 1 or len(xy1) != len(xy2):
        raise ValueError("model 0 / 1, at least one model and one match")
    N = len(xy1)
    return M, xy1, xy2, N, np.zeros(len(M), np.float32), np.zeros((len(M), (N + 31) // 32), np.uint32)


def score_host(model: int, M, xy1, xy2, sigma):
    """CheckHomography (model 0) / CheckFundamental (1) of given models on the host: (score[n], inlier flags (n, N))"""
    M, xy1, xy2, N, score, mask = _score_args(model, M, xy1, xy2)
    if _host().ccmh_twoview_score_host(model, len(M), _p(M), N, _p(xy1), _p(xy2), float(sigma), _p(score), _p(mask)) != 0:
        raise CcmError("ccmh_twoview_score_host: bad arguments")
    return score, mask_bits(mask, N)


def score_device(ctx: Context, model: int, M, xy1, xy2, sigma):
    """The same on the device through the test hook ccm_debug_twoview_score"""
    M, xy1, xy2, N, score, mask = _score_args(model, M, xy1, xy2)
    check(hooks().ccm_debug_twoview_score(ctx.handle, model, len(M), _p(M), N, _p(xy1), _p(xy2), C.c_float(sigma), _p(score), _p(mask)), ctx.handle)
    return score, mask_bits(mask, N)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the flat calls
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _ransac_out(N, H):
    w = (max(N, 1) + 31) // 32
    H = max(H, 1)
    return (np.zeros(H, np.float32), np.zeros(H, np.float32), np.zeros((H, 3, 3), np.float32), np.zeros((H, 3, 3), np.float32), np.zeros((H, w), np.uint32),
            np.zeros((H, w), np.uint32))


def _ransac_in(xy1, xy2, pn1, pn2, T1, T2inv, T2t, sets):
    a = [_f32(x, (-1, 2)) for x in (xy1, xy2, pn1, pn2)] + [_f32(x) for x in (T1, T2inv, T2t)]
    sets = _i32(sets, (-1, 8))
    if len({len(x) for x in a[:4]}) != 1 or any(x.size != 9 for x in a[4:]):
        raise ValueError("xy1, xy2, pn1, pn2 hold one x y pair per match; T1, T2inv, T2t are 3x3")
    return a, sets


def ransac_eval(ctx: Context, xy1, xy2, pn1, pn2, T1, T2inv, T2t, sigma, sets):
    """ccm_twoview_ransac_eval.  Returns (scoreH[H], scoreF[H], H21 (H, 3, 3), F21 (H, 3, 3), inliersH (H, N) bool, inliersF (H, N) bool)."""
    a, sets = _ransac_in(xy1, xy2, pn1, pn2, T1, T2inv, T2t, sets)
    N, H = len(a[0]), len(sets)
    o = _ransac_out(N, H)
    check(lib().ccm_twoview_ransac_eval(ctx.handle, N, *(_p(x) for x in a), C.c_float(sigma), H, _p(sets), *(_p(x) for x in o)), ctx.handle)
    return o[0], o[1], o[2], o[3], mask_bits(o[4], N), mask_bits(o[5], N)


def ransac_eval_host(xy1, xy2, pn1, pn2, T1, T2inv, T2t, sigma, sets, model: int = 0):
    """The same arguments through twoview_math.h compiled for the host, on the calling thread.  model 1 / 2: the homography / the fundamental matrix alone."""
    a, sets = _ransac_in(xy1, xy2, pn1, pn2, T1, T2inv, T2t, sets)
    N, H = len(a[0]), len(sets)
    o = _ransac_out(N, H)
    rc = _host().ccmh_twoview_ransac_eval_host(N, *(_p(x) for x in a), float(sigma), H, _p(sets), int(model), *(_p(x) for x in o))
    if rc != 0:
        raise CcmError(f"ccmh_twoview_ransac_eval_host: bad arguments ({rc})")
    return o[0], o[1], o[2], o[3], mask_bits(o[4], N), mask_bits(o[5], N)


def _rt_in(rec, K, xy1, xy2, inliers):
    rec = _f32(rec, (-1, REC_FLOATS)); K = _f32(K); xy1 = _f32(xy1, (-1, 2)); xy2 = _f32(xy2, (-1, 2))
    N, Q = len(xy1), len(rec)
    if K.size != 9 or len(xy2) != N or np.asarray(inliers).size != N:
        raise ValueError("K is 3x3; xy1, xy2 and inliers hold one entry per match")
    mask = bits_mask(inliers) if N else np.zeros(1, np.uint32)
    return rec, K, xy1, xy2, mask, N, Q, np.zeros(max(N * Q, 1), np.uint8), np.zeros((max(N * Q, 1), 3), np.float32), np.zeros(max(N * Q, 1), np.float32)


def check_rt(ctx: Context, rec, K, xy1, xy2, inliers, th2):
    """ccm_twoview_check_rt.  Returns (status (Q, N) u8, x3d (Q, N, 3), cosParallax (Q, N))."""
    rec, K, xy1, xy2, mask, N, Q, st, x, c = _rt_in(rec, K, xy1, xy2, inliers)
    check(lib().ccm_twoview_check_rt(ctx.handle, Q, _p(rec), _p(K), N, _p(xy1), _p(xy2), _p(mask), C.c_float(th2), _p(st), _p(x), _p(c)), ctx.handle)
    return st[:N * Q].reshape(Q, N), x[:N * Q].reshape(Q, N, 3), c[:N * Q].reshape(Q, N)


def check_rt_host(rec, K, xy1, xy2, inliers, th2):
    rec, K, xy1, xy2, mask, N, Q, st, x, c = _rt_in(rec, K, xy1, xy2, inliers)
    rc = _host().ccmh_twoview_check_rt_host(Q, _p(rec), _p(K), N, _p(xy1), _p(xy2), _p(mask), float(th2), _p(st), _p(x), _p(c))
    if rc != 0:
        raise CcmError(f"ccmh_twoview_check_rt_host: bad arguments ({rc})")
    return st[:N * Q].reshape(Q, N), x[:N * Q].reshape(Q, N, 3), c[:N * Q].reshape(Q, N)


def draw_sets(N: int, iterations: int, raw) -> np.ndarray:
    """The set-drawing loop of Initializer.cpp:73-93 on 8 * iterations raw rand() values: (iterations, 8) match indices"""
    raw = _i32(raw)
    if raw.size < 8 * iterations:
        raise ValueError("8 raw values per iteration")
    sets = np.zeros((max(iterations, 1), 8), np.int32)
    if _host().ccmh_twoview_draw_sets(int(N), int(iterations), _p(raw), _p(sets)) != 0:
        raise CcmError("ccmh_twoview_draw_sets: fewer than 8 matches")
    return sets[:iterations]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# cslam::TwoViewInitializer
# ---------------------------------------------------------------------------------------------------------------------------------------------
class TwoViewInitializer:
    """cslam::TwoViewInitializer.  keys1: (N1, 2) mvKeysUn of the reference frame.  device=None asks for the host evaluator by name (no device is touched)."""

    def __init__(self, device: Optional[int], K, keys1, sigma: float = 1.0):
        K = _f32(K); self._keys1 = _f32(keys1, (-1, 2))
        self._h = _host().ccmh_twoview_create(-1 if device is None else int(device), _p(K), len(self._keys1), _p(self._keys1), float(sigma))
        if not self._h:
            raise CcmError("ccmh_twoview_create failed (bad arguments or no device)")
        self.n_matches = 0

    def find(self, keys2, matches12, sets) -> dict:
        """FindHomography + FindFundamental: SH, SF, RH, H21, F21, bestH, bestF (-1: no winner), inliersH, inliersF (one flag per match)"""
        keys2 = _f32(keys2, (-1, 2)); m12 = _i32(matches12); sets = _i32(sets, (-1, 8))
        if m12.size != len(self._keys1):
            raise ValueError("matches12 holds one entry per keypoint of frame 1")
        n = int((m12 >= 0).sum())
        sc = np.zeros(3, np.float32); best = np.zeros(2, np.int32); H21 = np.zeros((3, 3), np.float32); F21 = np.zeros((3, 3), np.float32)
        ih = np.zeros(max(n, 1), np.uint8); i_f = np.zeros(max(n, 1), np.uint8)
        rc = _host().ccmh_twoview_find(self._h, len(keys2), _p(keys2), _p(m12), len(sets), _p(sets), _p(sc), _p(best), _p(H21), _p(F21), _p(ih), _p(i_f))
        if rc < 0:
            raise CcmError(f"ccmh_twoview_find failed ({rc})")
        self.n_matches = rc
        return dict(SH=sc[0], SF=sc[1], RH=sc[2], H21=H21, F21=F21, bestH=int(best[0]), bestF=int(best[1]), inliersH=ih[:rc].astype(bool), inliersF=i_f[:rc].astype(bool))

    def check_rt_batch(self, R, t, inliers, th2):
        """CheckRT of 1..8 hypotheses: a list of dicts nGood, parallax, vP3D (N1, 3), vbGood (N1,), status (matches,)"""
        R = _f32(R, (-1, 9)); t = _f32(t, (-1, 3)); Q = len(R)
        Rt = np.ascontiguousarray(np.concatenate([R, t], 1)); inl = np.ascontiguousarray(np.asarray(inliers, np.uint8).reshape(-1))
        N1, N = len(self._keys1), self.n_matches
        if inl.size != N or len(t) != Q or not 1 <= Q <= 8:
            raise ValueError("1 to 8 hypotheses, one inlier flag per match of the last find()")
        ng = np.zeros(Q, np.int32); par = np.zeros(Q, np.float32); p3d = np.zeros((Q, N1, 3), np.float32); good = np.zeros((Q, N1), np.uint8)
        st = np.zeros((Q, max(N, 1)), np.uint8)
        rc = _host().ccmh_twoview_check_rt(self._h, Q, _p(Rt), _p(inl), float(th2), _p(ng), _p(par), _p(p3d), _p(good), _p(st))
        if rc != 0:
            raise CcmError(f"ccmh_twoview_check_rt failed ({rc})")
        return [dict(nGood=int(ng[q]), parallax=par[q], vP3D=p3d[q], vbGood=good[q].astype(bool), status=st.reshape(Q, -1)[q, :N]) for q in range(Q)]

    def close(self):
        if getattr(self, "_h", None):
            _host().ccmh_twoview_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------------------
YAW_DEG = 3.0
T21 = (-0.3, 0.02, 0.05)


def motion():
    """(R21, t21) of the scenes in f64: 3 degrees of yaw (about the camera's y axis) and T21"""
    a = np.deg2rad(YAW_DEG)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return R, np.array(T21, np.float64)


def make_scene(kind: str, N: int, seed: int = 0, noise_px: float = 0.5, unmatched: int = 0, outliers: float = 0.0, K=synth.EUROC_K) -> dict:
    """kind "planar": points on the tilted plane z = 6 + 0.3 x; "general": depths 4-12.  N matches, `unmatched` more keypoints per frame that have no match
    (Normalize still sees them), a share `outliers` of the matches with a random second keypoint.  Frame 2 numbers its keypoints in its own order.
    Returns keys1 (N1, 2), keys2 (N2, 2), matches12 (N1,), xy1 / xy2 (N, 2) in match order, K (3, 3), R, t (f32), X (N, 3)."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    R, t = motion()
    px = np.stack([rng.uniform(30, synth.IMG_W - 30, N), rng.uniform(30, synth.IMG_H - 30, N)], 1)
    ax, ay = (px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy
    if kind == "planar":
        z = 6.0 / (1.0 - 0.3 * ax)                       # z = 6 + 0.3 x with x = ax z
    elif kind == "general":
        z = rng.uniform(4.0, 12.0, N)
    else:
        raise ValueError(kind)
    X = np.stack([ax * z, ay * z, z], 1)
    X2 = X @ R.T + t
    p2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
    p1 = px + rng.normal(0, noise_px, (N, 2)); p2 = p2 + rng.normal(0, noise_px, (N, 2))
    bad = rng.random(N) < outliers
    p2[bad] = np.stack([rng.uniform(0, synth.IMG_W, int(bad.sum())), rng.uniform(0, synth.IMG_H, int(bad.sum()))], 1)
    extra = lambda: np.stack([rng.uniform(0, synth.IMG_W, unmatched), rng.uniform(0, synth.IMG_H, unmatched)], 1)
    keys1 = np.concatenate([p1, extra()]); order1 = rng.permutation(len(keys1))
    keys2 = np.concatenate([p2, extra()]); order2 = rng.permutation(len(keys2))
    keys1 = keys1[order1].astype(np.float32); keys2 = keys2[order2].astype(np.float32)
    inv2 = np.argsort(order2)
    matches12 = np.full(len(keys1), -1, np.int32)
    src = order1 < N                                   # keypoint i of frame 1 is match order1[i]
    matches12[src] = inv2[order1[src]]
    i1 = np.nonzero(matches12 >= 0)[0]
    return dict(keys1=keys1, keys2=keys2, matches12=matches12, xy1=keys1[i1], xy2=keys2[matches12[i1]], first=i1.astype(np.int32), K=K_matrix(K),
                R=R.astype(np.float32), t=t.astype(np.float32), X=X[order1[i1]])


def ransac_inputs(sc: dict):
    """The positional arguments of ransac_eval / ransac_eval_host up to T2t for a scene: Normalize over all keypoints, then the matched ones in match order"""
    n1, T1 = normalize(sc["keys1"]); n2, T2 = normalize(sc["keys2"])
    i1 = sc["first"]
    return sc["xy1"], sc["xy2"], n1[i1], n2[sc["matches12"][i1]], T1, inv33(T2), np.ascontiguousarray(T2.T)


def random_sets(N: int, H: int, seed: int = 0) -> np.ndarray:
    """H sets drawn as the reference draws them, from a seeded stream of raw values in [0, RAND_MAX]"""
    raw = np.random.default_rng(seed).integers(0, 2**31 - 1, 8 * H, dtype=np.int64).astype(np.int32)
    return draw_sets(N, H, raw)


def motion_hypotheses(sc: dict, n: int):
    """n <= 8 (R, t) pairs: the true motion first, then the twisted pair and sign flips a decomposition would propose"""
    R, t = sc["R"].astype(np.float64), sc["t"].astype(np.float64)
    tn = t / np.linalg.norm(t)
    Rpi = 2 * np.outer(tn, tn) - np.eye(3)             # rotation by pi about the baseline
    a = np.deg2rad(11.0)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    cand = [(R, tn), (R, -tn), (Rpi @ R, tn), (Rpi @ R, -tn), (Rz @ R, tn), (R, np.array([0, 0, 1.0])), (np.eye(3), tn), (R.T, -tn)]
    Rs = np.stack([c[0] for c in cand[:n]]).astype(np.float32).reshape(n, 9)
    ts = np.stack([c[1] for c in cand[:n]]).astype(np.float32)
    return Rs, ts
