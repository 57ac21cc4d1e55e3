"""Bundle-adjustment / pose-optimisation entry points of the C ABI (Optimizer path).

Python harness over ccm_ba_* / ccm_pose_optimize (include/ccm_hip.h), mirroring the static methods
of cslam::Optimizer on flat problems:
  local_bundle_adjustment  <- Optimizer::LocalBundleAdjustmentClient (cslam/src/Optimizer.cpp:349-644)
  global_bundle_adjustment <- Optimizer::MapFusionGBA                (cslam/src/Optimizer.cpp:646-859)
  pose_optimization        <- Optimizer::PoseOptimizationClient      (cslam/src/Optimizer.cpp:215-347)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import BAOptions, BAProblem, BAStats, Context, check, hooks, lib


TRIAL_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p).value if a is not None else None


class BAHandle:
    """Staged BA (ccm_ba_create / run / download).  Keeps the flattened arrays alive."""

    def __init__(self, ctx: Context, prob: dict, rank: int = 0, nranks: int = 1, resident: "ResidentProblem | None" = None):
        """resident: the flat problem already uploaded to HBM (ResidentProblem): ccm_ba_create then reads device memory only."""
        self.ctx = ctx
        self.prob = prob
        if resident is not None:
            self._keep = resident.keep
            self.cprob = resident.host_cprob
            self._h = C.c_void_p()
            check(lib().ccm_ba_create(ctx.handle, C.byref(resident.dev_cprob), int(rank), int(nranks), C.byref(self._h)), ctx.handle)
            ctx.adopt(self)
            return
        self._keep = {
            "cam_qt": np.ascontiguousarray(prob["cam_qt"], np.float64).copy(),
            "cam_fixed": np.ascontiguousarray(prob["cam_fixed"], np.uint8),
            "cam_K": np.ascontiguousarray(prob["cam_K"], np.float64),
            "pt_xyz": np.ascontiguousarray(prob["pt_xyz"], np.float64).copy(),
            "e_cam": np.ascontiguousarray(prob["e_cam"], np.int32),
            "e_pt": np.ascontiguousarray(prob["e_pt"], np.int32),
            "e_obs": np.ascontiguousarray(prob["e_obs"], np.float64),
            "e_info": np.ascontiguousarray(prob["e_info"], np.float64),
        }
        lvl = prob.get("e_level")
        self._keep["e_level"] = np.ascontiguousarray(lvl, np.uint8) if lvl is not None else None
        k = self._keep
        self.cprob = BAProblem(int(prob["n_cam"]), int(prob["n_pt"]), int(prob["n_edge"]), _vp(k["cam_qt"]),
                               _vp(k["cam_fixed"]), _vp(k["cam_K"]), _vp(k["pt_xyz"]), _vp(k["e_cam"]), _vp(k["e_pt"]),
                               _vp(k["e_obs"]), _vp(k["e_info"]), _vp(k["e_level"]), float(prob["huber_delta"]))
        self._h = C.c_void_p()
        check(lib().ccm_ba_create(ctx.handle, C.byref(self.cprob), int(rank), int(nranks), C.byref(self._h)), ctx.handle)
        ctx.adopt(self)

    def reset(self):
        check(lib().ccm_ba_reset_state(self._h, C.c_void_p(_vp(self._keep["cam_qt"])), C.c_void_p(_vp(self._keep["pt_xyz"]))),
              self.ctx.handle)

    def push_state(self):
        """SparseOptimizer::push(): keep a device-side copy of the current estimate"""
        check(lib().ccm_ba_push_state(self._h), self.ctx.handle)

    def pop_state(self):
        """SparseOptimizer::pop(): the saved estimate becomes current again (device-to-device, stream-ordered)"""
        check(lib().ccm_ba_pop_state(self._h), self.ctx.handle)

    def run(self, max_iters: int, pcg_max_iters: int = 0, pcg_rel_tol: float = 0.0, lambda_init: float = 0.0,
            verbose: int = 0, stop_flag=None) -> BAStats:
        """optimizer.optimize(max_iters).  stop_flag: a 1-element numpy uint8 array playing the reference's bool* pbStopFlag."""
        opt = BAOptions(int(max_iters), int(pcg_max_iters), float(pcg_rel_tol), float(lambda_init), int(verbose))
        st = BAStats()
        fl = stop_flag.ctypes.data_as(C.c_void_p) if stop_flag is not None else None
        check(lib().ccm_ba_run(self._h, C.byref(opt), fl, C.byref(st)), self.ctx.handle)
        return st

    def set_edge_levels(self, e_level, huber_delta: float):
        """second stage of the local BA on the same handle (ccm_ba_set_edge_levels): edges with level != 0 leave, new Huber delta"""
        lvl = np.ascontiguousarray(e_level, np.uint8)
        check(lib().ccm_ba_set_edge_levels(self._h, C.c_void_p(_vp(lvl)), C.c_double(huber_delta)), self.ctx.handle)

    def history(self):
        """(chi2 after each LM iteration, lambda after it, trials it took) of the last run"""
        n = C.c_int(0)
        chi, lam, tr = np.zeros(256), np.zeros(256), np.zeros(256, np.int32)
        check(lib().ccm_ba_history(self._h, 256, C.c_void_p(_vp(chi)), C.c_void_p(_vp(lam)), C.c_void_p(_vp(tr)), C.byref(n)), self.ctx.handle)
        k = min(n.value, 256)
        return chi[:k].copy(), lam[:k].copy(), tr[:k].copy()

    def set_trial_callback(self, fn):
        """fn(iteration, trial_in_iteration, chi2_trial, accepted) after every LM trial, on the optimising thread; None removes it"""
        if fn is None:
            self._cb = None
            check(lib().ccm_ba_set_trial_callback(self._h, None, None), self.ctx.handle)
            return
        self._cb = TRIAL_CB(lambda user, it, tr, chi, acc: fn(it, tr, chi, acc))
        check(lib().ccm_ba_set_trial_callback(self._h, self._cb, None), self.ctx.handle)

    def download(self, chi2_in=None):
        cam = self._keep["cam_qt"].copy()
        pts = self._keep["pt_xyz"].copy()
        ne = int(self.prob["n_edge"])
        chi2 = np.zeros(ne, np.float64) if chi2_in is None else np.ascontiguousarray(chi2_in, np.float64).copy()
        dpos = np.zeros(ne, np.uint8)
        check(lib().ccm_ba_download(self._h, C.c_void_p(_vp(cam)), C.c_void_p(_vp(pts)), C.c_void_p(_vp(chi2))),
              self.ctx.handle)
        check(lib().ccm_ba_depth_positive(C.byref(self.cprob), C.c_void_p(_vp(cam)), C.c_void_p(_vp(pts)),
                                          C.c_void_p(_vp(dpos))), self.ctx.handle)
        return cam, pts, chi2, dpos

    def counts(self):
        v = [C.c_int64() for _ in range(5)]
        check(lib().ccm_ba_counts(self._h, *[C.byref(x) for x in v]), self.ctx.handle)
        return dict(zip(("edges", "points", "free_cams", "blocks", "pairs"), (x.value for x in v)))

    def partial_reduced(self, lam: float) -> np.ndarray:
        """Test hook: this rank's partial [S | b_schur] at the current state (ccm_ba_debug_partial_reduced)."""
        n = C.c_size_t()
        check(hooks().ccm_ba_debug_partial_reduced(self._h, C.c_double(lam), None, C.c_size_t(0), C.byref(n)), self.ctx.handle)
        out = np.zeros(n.value, np.float64)
        check(hooks().ccm_ba_debug_partial_reduced(self._h, C.c_double(lam), C.c_void_p(_vp(out)), C.c_size_t(out.size), C.byref(n)),
              self.ctx.handle)
        return out

    SIZES = ("Cp", "Lp", "Lloc", "Eloc", "nOff", "max_cam_edges", "row_units_max", "pers_grid", "coarse_na", "coarse_ncb", "n_chunk", "lp_begin")

    def debug_sizes(self) -> dict:
        """Test hook: the twelve `sizes` fields of ccm_ba_debug_array by name (row_units_max > 0: the row Schur kernel is in use; n_chunk > 0: the
        edge-parallel linearisation / back-substitution; lp_begin, Lloc: this rank's landmark slots)."""
        v = np.zeros(len(self.SIZES), np.int32)
        n = C.c_size_t(0)
        check(hooks().ccm_ba_debug_array(self._h, b"sizes", C.c_void_p(_vp(v)), C.c_size_t(v.nbytes), C.byref(n)), self.ctx.handle)
        assert n.value == v.nbytes
        return dict(zip(self.SIZES, (int(x) for x in v)))

    def coarse_level(self, lam: float):
        """Test hook (ccm_ba_debug_coarse): (na camera intervals, Ac, Ainv over the na + 1 coarse nodes, P) of the two-level preconditioner, or (0, None, None, None)."""
        na = C.c_int(0)
        check(hooks().ccm_ba_debug_coarse(self._h, C.c_double(lam), C.byref(na), None, None, None, C.c_size_t(0)), self.ctx.handle)
        if na.value == 0:
            return 0, None, None, None
        nc = 6 * (na.value + 1)
        Ac = np.zeros((nc, nc)); Ai = np.zeros((nc, nc)); P = np.zeros((self.counts()["free_cams"], 6, 6))
        check(hooks().ccm_ba_debug_coarse(self._h, C.c_double(lam), C.byref(na), C.c_void_p(_vp(Ac)), C.c_void_p(_vp(Ai)), C.c_void_p(_vp(P)),
                                        C.c_size_t(Ac.size)), self.ctx.handle)
        return na.value, Ac, Ai, P

    def close(self):
        if self._h:
            lib().ccm_ba_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResidentProblem:
    """The flat arrays of a BA problem uploaded once to HBM; `dev_cprob` is a ccm_ba_problem whose pointers address device memory
    (ccm_ba_create accepts either, include/ccm_hip.h)."""

    def __init__(self, ctx: Context, prob: dict):
        self.ctx = ctx
        k = self.keep = {
            "cam_qt": np.ascontiguousarray(prob["cam_qt"], np.float64).copy(), "cam_fixed": np.ascontiguousarray(prob["cam_fixed"], np.uint8),
            "cam_K": np.ascontiguousarray(prob["cam_K"], np.float64), "pt_xyz": np.ascontiguousarray(prob["pt_xyz"], np.float64).copy(),
            "e_cam": np.ascontiguousarray(prob["e_cam"], np.int32), "e_pt": np.ascontiguousarray(prob["e_pt"], np.int32),
            "e_obs": np.ascontiguousarray(prob["e_obs"], np.float64), "e_info": np.ascontiguousarray(prob["e_info"], np.float64),
            "e_level": np.ascontiguousarray(prob["e_level"], np.uint8) if prob.get("e_level") is not None else None}
        order = ("cam_qt", "cam_fixed", "cam_K", "pt_xyz", "e_cam", "e_pt", "e_obs", "e_info", "e_level")
        self.dptr = {n: (ctx.upload(k[n]) if k[n] is not None else None) for n in order}
        dims = (int(prob["n_cam"]), int(prob["n_pt"]), int(prob["n_edge"]))
        self.host_cprob = BAProblem(*dims, *[_vp(k[n]) for n in order], float(prob["huber_delta"]))
        self.dev_cprob = BAProblem(*dims, *[self.dptr[n] for n in order], float(prob["huber_delta"]))
        self.bytes = sum(k[n].nbytes for n in order if k[n] is not None)

    def close(self):
        for p in self.dptr.values():
            if p:
                self.ctx.free(p)
        self.dptr = {}


def bundle_adjustment(ctx: Context, prob: dict, max_iters: int, chi2_in=None, **kw):
    """optimizer.initializeOptimization(0); optimizer.optimize(max_iters) on the flat problem.
    Returns (cam_qt, pt_xyz, chi2_per_edge, depth_pos, stats)."""
    h = BAHandle(ctx, prob)
    try:
        st = h.run(max_iters, **kw)
        cam, pts, chi2, dpos = h.download(chi2_in)
    finally:
        h.close()
    return cam, pts, chi2, dpos, st


def global_bundle_adjustment(ctx: Context, prob: dict, n_iterations: int = 20, **kw):
    """Optimizer::MapFusionGBA numerics (Optimizer.cpp:786-797): one optimize(nIterations) pass,
    Huber sqrt(5.99) on every edge."""
    return bundle_adjustment(ctx, prob, n_iterations, **kw)


def local_bundle_adjustment(ctx: Context, prob: dict, **kw):
    """Optimizer::LocalBundleAdjustmentClient numerics (Optimizer.cpp:536-602): optimize(5) with Huber
    sqrt(5.991); edges with chi2 > 5.991 or non-positive depth go to level 1 and the kernel is
    dropped; optimize(10); finally every edge with chi2 > 5.991 or non-positive depth is reported
    for erasure (level-1 edges keep the chi2 of the first pass, as g2o leaves their _error alone).
    Returns (cam_qt, pt_xyz, to_erase mask, stats1, stats2)."""
    p1 = dict(prob)
    p1["huber_delta"] = float(np.float32(np.sqrt(np.float32(5.991))))
    level = np.ascontiguousarray(prob.get("e_level") if prob.get("e_level") is not None else np.zeros(prob["n_edge"], np.uint8), np.uint8).copy()
    active = level == 0
    if kw.pop("one_handle", True):
        # both stages on ONE handle (what shim/Optimizer_hip.cpp does): the outliers of the first pass leave through ccm_ba_set_edge_levels
        h = BAHandle(ctx, p1)
        try:
            st1 = h.run(5, **kw)
            _, _, chi2, dpos = h.download()
            level[active & ((chi2 > 5.991) | (dpos == 0))] = 1
            h.set_edge_levels(level, 0.0)
            st2 = h.run(10, **kw)
            cam2, pts2, chi2b, dpos2 = h.download(chi2)
        finally:
            h.close()
        erase = active & ((chi2b > 5.991) | (dpos2 == 0))
        return cam2, pts2, erase, st1, st2
    cam, pts, chi2, dpos, st1 = bundle_adjustment(ctx, p1, 5, **kw)
    out = active & ((chi2 > 5.991) | (dpos == 0))
    level[out] = 1
    p2 = dict(prob)
    p2.update(cam_qt=cam, pt_xyz=pts, e_level=level, huber_delta=0.0)
    cam2, pts2, chi2b, dpos2, st2 = bundle_adjustment(ctx, p2, 10, chi2_in=chi2, **kw)
    erase = active & ((chi2b > 5.991) | (dpos2 == 0))
    return cam2, pts2, erase, st1, st2


def pose_optimization(ctx: Context, cam_qt, Xw, obs, info, K):
    cam = np.ascontiguousarray(cam_qt, np.float64).copy()
    Xw = np.ascontiguousarray(Xw, np.float64)
    obs = np.ascontiguousarray(obs, np.float64)
    info = np.ascontiguousarray(info, np.float64)
    K = np.ascontiguousarray(K, np.float64)
    n = Xw.shape[0]
    outl = np.zeros(max(n, 1), np.uint8)
    ninl = C.c_int(0)
    check(lib().ccm_pose_optimize(ctx.handle, C.c_void_p(_vp(cam)), n, C.c_void_p(_vp(Xw)), C.c_void_p(_vp(obs)),
                                  C.c_void_p(_vp(info)), C.c_void_p(_vp(K)), C.c_void_p(_vp(outl)), C.byref(ninl)),
          ctx.handle)
    return cam, outl[:n], ninl.value


class PoseOptCall:
    """Call object for ccm_pose_optimize: arguments converted once; run() restores the initial pose (7 doubles) and makes exactly one C-ABI call
    (bench.py times this; pose_optimization() above spends ~10 us per call in numpy / ctypes conversions).  Results: .cam, .outlier, .n_inlier."""

    def __init__(self, ctx: Context, cam_qt, Xw, obs, info, K):
        f = lambda a: np.ascontiguousarray(a, np.float64)
        self.ctx = ctx
        self._cam0 = f(cam_qt).copy()
        self.cam = self._cam0.copy()
        self._in = (f(Xw), f(obs), f(info), f(K))
        n = self._in[0].shape[0]
        self.n = n
        self.outlier = np.zeros(max(n, 1), np.uint8)
        self._ninl = C.c_int(0)
        v = lambda a: C.c_void_p(_vp(a))
        self._args = (ctx.handle, v(self.cam), n, v(self._in[0]), v(self._in[1]), v(self._in[2]), v(self._in[3]), v(self.outlier), C.byref(self._ninl))
        self._fn = lib().ccm_pose_optimize

    def run(self):
        self.cam[:] = self._cam0
        rc = self._fn(*self._args)
        if rc:
            check(rc, self.ctx.handle)

    @property
    def n_inlier(self):
        return self._ninl.value


def sim3_optimization(ctx: Context, sim3, P1c, P2c, obs1, obs2, info1, info2, K1, K2, th2: float = 10.0, fix_scale: bool = False):
    """Optimizer::OptimizeSim3 (Optimizer.cpp:861-1056) through ccm_sim3_optimize.  Returns (sim3[8], inlier flags, nIn)."""
    f = lambda a: np.ascontiguousarray(a, np.float64)
    s = f(sim3).copy()
    P1c, P2c, obs1, obs2, info1, info2, K1, K2 = map(f, (P1c, P2c, obs1, obs2, info1, info2, K1, K2))
    n = P1c.shape[0] if P1c.ndim == 2 else P1c.size // 3
    inl = np.zeros(max(n, 1), np.uint8)
    nin = C.c_int(0)
    v = lambda a: C.c_void_p(_vp(a))
    check(lib().ccm_sim3_optimize(ctx.handle, v(s), n, v(P1c), v(P2c), v(obs1), v(obs2), v(info1), v(info2), v(K1), v(K2),
                                  C.c_double(th2), int(bool(fix_scale)), v(inl), C.byref(nin)), ctx.handle)
    return s, inl[:n], nin.value


class PGStats(C.Structure):
    _fields_ = [("iters_done", C.c_int32), ("lm_trials", C.c_int32), ("pcg_iters", C.c_int32), ("reserved", C.c_int32),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double)]


def pose_graph_optimization(ctx: Context, pg: dict, max_iters: int = 20, lambda_init: float = 1e-16):
    """OptimizeEssentialGraph{LoopClosure,MapFusion} numerics (Optimizer.cpp:1058-1566) through ccm_pose_graph_optimize.
    pg: sim3[n,8], fixed[n], fix_scale, e_i, e_j, meas[m,8] (synth.make_pose_graph layout).  Returns (sim3, stats)."""
    sim3 = np.ascontiguousarray(pg["sim3"], np.float64).copy()
    fixed = np.ascontiguousarray(pg["fixed"], np.uint8)
    e_i, e_j = np.ascontiguousarray(pg["e_i"], np.int32), np.ascontiguousarray(pg["e_j"], np.int32)
    meas = np.ascontiguousarray(pg["meas"], np.float64)
    st = PGStats()
    v = lambda a: C.c_void_p(_vp(a))
    check(lib().ccm_pose_graph_optimize(ctx.handle, int(sim3.shape[0]), v(sim3), v(fixed), int(bool(pg["fix_scale"])), int(e_i.size), v(e_i), v(e_j),
                                        v(meas), int(max_iters), C.c_double(lambda_init), None, C.byref(st)), ctx.handle)
    return sim3, st


class PGDebugOut(C.Structure):
    """ccm_pg_debug_out of include/ccm_testhooks.h"""
    _fields_ = [("F", C.c_int32), ("nBlk", C.c_int32), ("E_active", C.c_int32), ("reserved", C.c_int32), ("flags", C.c_int32 * 4),
                ("cap_free", C.c_size_t), ("cap_edge", C.c_size_t), ("cap_blk", C.c_size_t),
                ("blk_a", C.c_void_p), ("blk_b", C.c_void_p), ("active", C.c_void_p),
                ("H", C.c_void_p), ("b", C.c_void_p), ("J", C.c_void_p), ("err", C.c_void_p), ("x", C.c_void_p), ("z_out", C.c_void_p),
                ("t_parent", C.c_void_p), ("t_code", C.c_void_p), ("t_order", C.c_void_p), ("t_pos", C.c_void_p), ("t_out", C.c_void_p)]


PG_SOLVERS = {"tiles": 0, "dense": 1, "forest": 2, "jacobi": 3}


def debug_pg_solve(ctx: Context, pg: dict, lam: float, solver, rel_tol: float = 1e-10, max_it: int = 1000, r_in=None):
    """Test hook (ccm_debug_pg_solve): one linearisation of pg at its state and one solve of (H + lam I) x = b by `solver` ("tiles", "dense", "forest",
    "jacobi" or 0..3), forced at any size.  Returns a dict: F, nBlk, keys[nBlk,2], H[nBlk,7,7], b[7F], J[E,2,7,7], err[E,7], active[E], x[7F], flags[4]
    (done, iterations, failure, stalled); for the forest solver t_parent, t_code, t_order, t_pos, t_out; with r_in, z = M^-1 r_in."""
    solver = PG_SOLVERS.get(solver, solver)
    sim3 = np.ascontiguousarray(pg["sim3"], np.float64)
    fixed = np.ascontiguousarray(pg["fixed"], np.uint8)
    e_i, e_j = np.ascontiguousarray(pg["e_i"], np.int32), np.ascontiguousarray(pg["e_j"], np.int32)
    meas = np.ascontiguousarray(pg["meas"], np.float64)
    F = int((fixed == 0).sum())
    E = int((~((fixed[e_i] != 0) & (fixed[e_j] != 0))).sum()) if e_i.size else 0
    cap_blk = F + E
    a = dict(blk_a=np.zeros(cap_blk, np.int32), blk_b=np.zeros(cap_blk, np.int32), active=np.zeros(E, np.int32), H=np.zeros(49 * cap_blk), b=np.zeros(7 * F),
             J=np.zeros(98 * E), err=np.zeros(7 * E), x=np.zeros(7 * F), z_out=np.zeros(7 * F))
    a.update({n: np.zeros(F, np.int32) for n in ("t_parent", "t_code", "t_order", "t_pos", "t_out")})
    out = PGDebugOut(cap_free=F, cap_edge=E, cap_blk=cap_blk, **{n: _vp(v) for n, v in a.items()})
    r = None if r_in is None else np.ascontiguousarray(r_in, np.float64)
    if r is not None and r.size != 7 * F:
        raise ValueError("r_in must hold 7 F values")
    v = lambda x: C.c_void_p(_vp(x))
    check(hooks().ccm_debug_pg_solve(ctx.handle, int(sim3.shape[0]), v(sim3), v(fixed), int(bool(pg["fix_scale"])), int(e_i.size), v(e_i), v(e_j), v(meas),
                                     C.c_double(lam), int(solver), C.c_double(rel_tol), int(max_it), None if r is None else v(r), C.byref(out)), ctx.handle)
    nB = out.nBlk
    res = dict(F=out.F, nBlk=nB, keys=np.stack([a["blk_a"][:nB], a["blk_b"][:nB]], axis=1), H=a["H"][:49 * nB].reshape(nB, 7, 7), b=a["b"],
               J=a["J"].reshape(E, 2, 7, 7), err=a["err"].reshape(E, 7), active=a["active"], x=a["x"], flags=np.array(list(out.flags), np.int32))
    if solver == 2:
        res.update({n: a[n] for n in ("t_parent", "t_code", "t_order", "t_pos", "t_out")})
    if r is not None:
        res["z"] = a["z_out"]
    return res


BLOCK_RED_CALLS = ("sum1", "sum28_lds", "sum28_lds", "sum1", "sum27", "sum27", "sum64", "sum64", "sum1")
BLOCK_RED_SLOTS = {"sum1": (1, 1), "sum28_lds": (32, 28), "sum27": (32, 28), "sum64": (64, 35)}   # (input slots, results) per thread


def debug_block_red(ctx: Context, inputs):
    """Test hook (ccm_debug_block_red): the sequence BLOCK_RED_CALLS on one BlockRedT<4> object in ONE launch of 256 threads.  inputs: one array [slots, 256] per
    call (slots as in BLOCK_RED_SLOTS); returns one array [results, 256] per call, the values EVERY thread ended with."""
    if len(inputs) != len(BLOCK_RED_CALLS):
        raise ValueError("one input array per call of BLOCK_RED_CALLS")
    flat = []
    for name, a in zip(BLOCK_RED_CALLS, inputs):
        a = np.ascontiguousarray(a, np.float64)
        if a.shape != (BLOCK_RED_SLOTS[name][0], 256):
            raise ValueError(f"{name}: input must be [{BLOCK_RED_SLOTS[name][0]}, 256]")
        flat.append(a.ravel())
    src = np.concatenate(flat)
    out = np.zeros(256 * sum(BLOCK_RED_SLOTS[n][1] for n in BLOCK_RED_CALLS))
    check(hooks().ccm_debug_block_red(ctx.handle, C.c_void_p(_vp(src)), C.c_size_t(src.size), C.c_void_p(_vp(out)), C.c_size_t(out.size)), ctx.handle)
    res, o = [], 0
    for name in BLOCK_RED_CALLS:
        k = BLOCK_RED_SLOTS[name][1]
        res.append(out[o:o + 256 * k].reshape(k, 256).copy())
        o += 256 * k
    return res


def debug_lane_ops(ctx: Context, v64, key64):
    """Test hook (ccm_debug_lane_ops): lanex::from_partner_c(v, off) for off = 1, 2, 4, 8, 16, 32 ([6, 64]) and lanex::wave_min_u32(key) of the 64 lanes ([64])."""
    v = np.ascontiguousarray(v64, np.float64); key = np.ascontiguousarray(key64, np.uint32)
    if v.shape != (64,) or key.shape != (64,):
        raise ValueError("64 lanes")
    partner = np.zeros((6, 64)); kmin = np.zeros(64, np.uint32)
    check(hooks().ccm_debug_lane_ops(ctx.handle, C.c_void_p(_vp(v)), C.c_void_p(_vp(key)), C.c_void_p(_vp(partner)), C.c_void_p(_vp(kmin))), ctx.handle)
    return partner, kmin


def debug_lie_eval(ctx: Context, op: int, x, out_init=None):
    """Test hook (ccm_debug_lie_eval): lie_eval(op, ...) of csrc/test_lie_ops.h on the device for the items x[n, 48], one lane each; returns out[n, 40]
    (out[:, 39] the flag word).  out_init: the values the outputs start from (default 0)."""
    x = np.ascontiguousarray(x, np.float64)
    if x.ndim != 2 or x.shape[1] != 48 or x.shape[0] < 1:
        raise ValueError("x must be [n, 48], n >= 1")
    out = np.zeros((x.shape[0], 40)) if out_init is None else np.ascontiguousarray(out_init, np.float64).copy()
    if out.shape != (x.shape[0], 40):
        raise ValueError("out_init must be [n, 40]")
    check(hooks().ccm_debug_lie_eval(ctx.handle, int(op), int(x.shape[0]), C.c_void_p(_vp(x)), C.c_void_p(_vp(out))), ctx.handle)
    return out


def debug_poseopt_linearise(ctx: Context, cam_qt, Xw, obs, info, K, level, robust):
    """Test hook (ccm_debug_poseopt_linearise): staging and ONE linearisation of the pose optimiser's kernel at cam_qt with the given level / robust bytes per edge.
    Returns a dict: acc[28, 256] (every thread's H upper triangle 0..20, b 21..26, robust chi2 27), err[n, 2], tr_red, use_lds, lds_bytes (the launch shape taken)."""
    f = lambda a: np.ascontiguousarray(a, np.float64)
    cam, Xw, obs, info, K = map(f, (cam_qt, Xw, obs, info, K))
    n = Xw.shape[0]
    level = np.ascontiguousarray(level, np.uint8); robust = np.ascontiguousarray(robust, np.uint8)
    if obs.shape != (n, 2) or info.shape != (n,) or level.shape != (n,) or robust.shape != (n,):
        raise ValueError("n edges: Xw[n, 3], obs[n, 2], info[n], level[n], robust[n]")
    acc = np.zeros((28, 256)); err = np.zeros((n, 2)); shape = (C.c_int * 3)()
    v = lambda a: C.c_void_p(_vp(a))
    check(hooks().ccm_debug_poseopt_linearise(ctx.handle, v(cam), n, v(Xw), v(obs), v(info), v(K), v(level), v(robust), v(acc), v(err), shape), ctx.handle)
    return dict(acc=acc, err=err, tr_red=bool(shape[0]), use_lds=bool(shape[1]), lds_bytes=int(shape[2]))


def debug_sim3opt_linearise(ctx: Context, sim3, P1c, P2c, obs1, obs2, info1, info2, K1, K2, th2, fix_scale, alive):
    """Test hook (ccm_debug_sim3opt_linearise): staging, chi2, perturbed estimates and ONE accumulation of the Sim3 optimiser's kernel at sim3 with the given alive bytes.
    Returns a dict: acc[35, 256] (every thread's H upper triangle 0..27, b 28..34), chi2[256], err[n, 4], pert[14, 2, 8] (perturbation 2 d / 2 d + 1 = +-delta e_d;
    the estimate, its inverse), J[n, 2, 2, 7] (pair, side, row, column), use_lds, lds_bytes (the launch shape taken)."""
    f = lambda a: np.ascontiguousarray(a, np.float64)
    s, P1c, P2c, obs1, obs2, info1, info2, K1, K2 = map(f, (sim3, P1c, P2c, obs1, obs2, info1, info2, K1, K2))
    n = P1c.shape[0]
    alive = np.ascontiguousarray(alive, np.uint8)
    if P2c.shape != (n, 3) or obs1.shape != (n, 2) or obs2.shape != (n, 2) or info1.shape != (n,) or info2.shape != (n,) or alive.shape != (n,):
        raise ValueError("n pairs: P1c[n, 3], P2c[n, 3], obs1[n, 2], obs2[n, 2], info1[n], info2[n], alive[n]")
    acc = np.zeros((35, 256)); chi2 = np.zeros(256); err = np.zeros((n, 4)); pert = np.zeros((14, 2, 8)); J = np.zeros((n, 2, 2, 7)); shape = (C.c_int * 2)()
    v = lambda a: C.c_void_p(_vp(a))
    check(hooks().ccm_debug_sim3opt_linearise(ctx.handle, v(s), n, v(P1c), v(P2c), v(obs1), v(obs2), v(info1), v(info2), v(K1), v(K2), C.c_double(th2),
                                              int(bool(fix_scale)), v(alive), v(acc), v(chi2), v(err), v(pert), v(J), shape), ctx.handle)
    return dict(acc=acc, chi2=chi2, err=err, pert=pert, J=J, use_lds=bool(shape[0]), lds_bytes=int(shape[1]))


def debug_dense_solve(ctx: Context, A, b):
    """Test hook: SPD solve through the device's blocked MFMA-f64 Cholesky (ccm_debug_dense_solve)."""
    A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64)
    x = np.zeros_like(b); info = C.c_int(0)
    check(hooks().ccm_debug_dense_solve(ctx.handle, C.c_void_p(_vp(A)), C.c_void_p(_vp(b)), int(b.size), C.c_void_p(_vp(x)), C.byref(info)), ctx.handle)
    return x, info.value


def debug_planned_solve(ctx: Context, A, b):
    """Test hook: the same solve with a tile plan built from A's non-zero 64 x 64 tiles (ccm_debug_planned_solve)."""
    A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64)
    x = np.zeros_like(b); info = C.c_int(0)
    check(hooks().ccm_debug_planned_solve(ctx.handle, C.c_void_p(_vp(A)), C.c_void_p(_vp(b)), int(b.size), C.c_void_p(_vp(x)), C.byref(info)), ctx.handle)
    return x, info.value


def debug_tile_solve(ctx: Context, A, b):
    """Test hook: SPD solve through the tile-sparse, level-scheduled Cholesky (ccm_debug_tile_solve); returns (x, info, levels, tiles)."""
    A = np.ascontiguousarray(A, np.float64); b = np.ascontiguousarray(b, np.float64)
    x = np.zeros_like(b); info = C.c_int(0); levels = C.c_int(0); tiles = C.c_int(0)
    check(hooks().ccm_debug_tile_solve(ctx.handle, C.c_void_p(_vp(A)), C.c_void_p(_vp(b)), int(b.size), C.c_void_p(_vp(x)), C.byref(info),
                                     C.byref(levels), C.byref(tiles)), ctx.handle)
    return x, info.value, levels.value, tiles.value


def debug_dense_inverse(ctx: Context, A):
    """Test hook: explicit SPD inverse through the tile kernels of dense_chol.hip (ccm_debug_dense_inverse)."""
    A = np.ascontiguousarray(A, np.float64)
    out = np.zeros_like(A); info = C.c_int(0)
    check(hooks().ccm_debug_dense_inverse(ctx.handle, C.c_void_p(_vp(A)), int(A.shape[0]), C.c_void_p(_vp(out)), C.byref(info)), ctx.handle)
    return out, info.value
