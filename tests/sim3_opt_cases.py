"""Problems shared by tests/test_sim3_threshold_cpu.py and tests/test_sim3_gpu.py (no test lives here; plain numpy, no GPU).

Every builder starts from synth.make_sim3_problem and varies its OUTPUT (synth itself is relied on bit for bit elsewhere): a second camera, gross outliers
on either keyframe's side, a fixed scale that is not 1, a residual planted where the oracle's own chi2 decision flips, and problems whose first pass leaves
exactly 10 or 9 survivors.  `oracle` is the imported oracle module (the oracle_lib fixture)."""
import ctypes as C
import functools

import numpy as np

from ccm_slam_amd import synth

K2_ALT = np.array([435.2, 436.1, 380.0, 250.0])    # second camera: clearly not synth.EUROC_K (458.654, 457.296, 367.215, 248.375)

# Launch shapes of ccm_sim3_optimize (csrc/sim3opt.hip, host part): the dynamic LDS is [kRedDoubles = 512 | kPertDoubles = 14 * 16 = 224] doubles = 5888 B, then per pair
# 16 doubles (P1c 3, P2c 3, obs1 2, obs2 2, info1, info2, err 4) + 2 flag bytes = 130 B, + 16 B:  lds_full = 5904 + 130 n.
#   n <=  458: lds_full <=  64 KiB, plain launch                        (5904 + 130 *  458 =  65 444 <=  65 536 <  65 574 = 5904 + 130 *  459)
#   n <= 1136: lds_full <= 150 KiB, dynamic-LDS limit raised, all in LDS  (5904 + 130 * 1136 = 153 584 <= 153 600 < 153 714 = 5904 + 130 * 1137)
#   n >= 1137: only the 5888 B head in LDS, the problem stays in global memory
LDS_HEAD = (512 + 224) * 8
LDS_PER_PAIR = 16 * 8 + 2


def lds_full(n):
    return LDS_HEAD + LDS_PER_PAIR * n + 16


N_PLAIN_MAX = (64 * 1024 - lds_full(0)) // LDS_PER_PAIR       # 458
N_LDS_MAX = (150 * 1024 - lds_full(0)) // LDS_PER_PAIR        # 1136
STAGING_EDGES = (N_PLAIN_MAX, N_PLAIN_MAX + 1, N_LDS_MAX, N_LDS_MAX + 1)

# The reference's own resolution, measured by tests/test_sim3_threshold_cpu.py (plain oracle build against the -O3 -march=native build of the same source) on
# sweep_cases(): see that test's docstring for the figures.
MUST_DELTAS = (1e-4, 1e-5)           # planted this far (relative) from the flip the two builds agree on every flag: the device must, too
COUNTED_DELTAS = (1e-6, 1e-7)        # closer, the reference disagrees with itself in REF_SHARE of the calls: run and counted
REF_SHARE = {1e-6: 1 / 302, 1e-7: 17 / 302}   # measured shares of the 302 planted calls per delta on which the two builds differ (99 of 302 at 1e-8)
# largest build-to-build difference of a Sim3 component over the must cases with identical flags and nIn >= 16: 1.01e-5, on one problem of 700 pairs planted at 1e-4 and
# at 1e-5 (as generated the same problem gives 4.2e-7, which is also the largest figure of all other cases)
REF_SPREAD = 1.01e-5
MIN_INLIERS_FOR_ESTIMATE = 16        # below, the estimate amplifies rounding (1.6e-6 at n = 10, 2.9e-5 at n = 11 between the builds) and is no observable
# device tolerance on the estimate: 4 x the build-to-build spread — the device departs from the plain oracle in three rounding-level ways (FMA contraction, summation
# order of H / b, libm), the two builds in one
EST_TOL = 4 * REF_SPREAD


def share_cap(delta):
    """largest share of the calls planted at a counted delta that may differ from the plain oracle: twice the share at which the oracle's two builds differ on the same
    calls, with a floor of 1 % at 1e-6 so that one call in a few hundred cannot decide"""
    return max(2 * REF_SHARE[delta], 0.01 if delta == 1e-6 else 0.0)


def planted_pair_differs(j, got, want):
    """two (sim3, flags, nIn) results of a call planted at a counted delta that do not agree: the difference starts at pair j, whose flag differs.  ("Only pair j's
    flag, and nIn by one" does NOT hold for a correct implementation, and not between the reference's own two builds: where pair j's decision differs after the FIRST
    pass, the second pass optimises another set of pairs — its estimate moves by ~1e-3 and takes other borderline pairs along (seen: pairs 46 and 264 of 300) —, and where
    pair j is the tenth survivor the gate of Optimizer.cpp:1015 turns it into the whole count (nIn 10 against 0).  only_planted_pair() counts the plain kind.)"""
    return got[1][j] != want[1][j]


def only_planted_pair(j, got, want):
    return np.array_equal(np.flatnonzero(got[1] != want[1]), [j]) and abs(got[2] - want[2]) == 1


def args(p, **kw):
    """the positional arguments of oracle.sim3_optimize / optimizer.sim3_optimization (after ctx)"""
    q = dict(p, **kw)
    return (q["sim3"], q["P1c"], q["P2c"], q["obs1"], q["obs2"], q["info1"], q["info2"], q["K1"], q["K2"], q["th2"], q["fix_scale"])


def fast_sim3(fast, p):
    """ora_sim3_optimize of another build of the oracle (oracle.fast_lib()); same return as oracle.sim3_optimize"""
    a = args(p)
    s = np.ascontiguousarray(a[0], np.float64).copy()
    arr = [np.ascontiguousarray(x, np.float64) for x in a[1:9]]
    n = arr[0].shape[0]
    inl = np.zeros(max(n, 1), np.uint8)
    fn = fast.ora_sim3_optimize
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_double, C.c_int, C.c_void_p]
    nin = fn(s.ctypes.data, n, *[x.ctypes.data for x in arr], float(a[9]), int(bool(a[10])), inl.ctypes.data)
    return s, inl[:n], int(nin)


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def two_camera(p, K2=K2_ALT):
    """the same problem with keyframe 2 seen through another camera: obs2 re-expressed under K2 (f32-rounded like synth's keypoints)"""
    K = p["K2"]
    x, y = (p["obs2"][:, 0] - K[2]) / K[0], (p["obs2"][:, 1] - K[3]) / K[1]
    K2 = np.array(K2, np.float64)
    return dict(p, obs2=_f32(np.stack([K2[0] * x + K2[2], K2[1] * y + K2[3]], 1)), K2=K2)


def plant_outliers(p, side, idx, rng):
    """gross offsets of 30 .. 60 px per axis (random signs) on the pairs idx, in obs1 (side 0) or obs2 (side 1)"""
    idx = np.asarray(idx, np.int64)
    key = "obs2" if side else "obs1"
    obs = p[key].copy()
    obs[idx] += rng.uniform(30.0, 60.0, (idx.size, 2)) * rng.choice([-1.0, 1.0], (idx.size, 2))
    return dict(p, **{key: _f32(obs)})


def with_scale(p, s):
    """a fix_scale problem (true scale 1, start scale 1) restated at the scale s: map 2 shrunk by 1 / s, so X1 = s R X2' + t holds for the same R, t and the same keypoints"""
    assert p["fix_scale"] and p["sim3"][7] == 1.0
    sim3, gt = p["sim3"].copy(), p["gt_sim3"].copy()
    sim3[7] = s; gt[7] = s
    return dict(p, P2c=_f32(p["P2c"] / s), sim3=sim3, gt_sim3=gt)


def sim3_project(sim3, P, K, inverse):
    """K-projection of S P (inverse False) or of S^-1 P"""
    R = synth.R_from_quat(np.asarray(sim3)[None, :4])[0]
    t, s = np.asarray(sim3)[4:7], sim3[7]
    X = (P - t) @ R / s if inverse else s * (P @ R.T) + t
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)


def planted(p, j, side, base, off, s):
    key = "obs2" if side else "obs1"
    obs = p[key].copy(); obs[j] = base + s * off
    return dict(p, **{key: obs})


def plant_at_threshold(oracle, p, j, side, th2, iters=60):
    """tests/test_poseopt_gpu.py::_plant for OptimizeSim3: bisection ON THE ORACLE of the scale s of pair j's offset (from its projection at the oracle's optimum, through S with K1
    on side 0, through S^-1 with K2 on side 1; fixed direction, length sqrt(th2 / info) at s = 1) at which the oracle's final inlier[j] flips.  Returns (base, off, lo, hi) with
    inlier(lo) = 1, inlier(hi) = 0 and hi / lo - 1 < 1e-13, or None when the flag is not 1 at 0.5 and 0 at 2."""
    p = dict(p, th2=th2)
    so, _, _ = oracle.sim3_optimize(*args(p))
    if side:
        base = sim3_project(so, p["P1c"][j:j + 1], p["K2"], True)[0]
        info = p["info2"][j]
    else:
        base = sim3_project(so, p["P2c"][j:j + 1], p["K1"], False)[0]
        info = p["info1"][j]
    off = np.array([0.7, -0.4])
    off = off / np.hypot(*off) * np.sqrt(th2 / info)

    def flag(s):
        return oracle.sim3_optimize(*args(planted(p, j, side, base, off, s)))[1][j]
    lo, hi = 0.5, 2.0
    if not np.all(np.isfinite(base)) or flag(lo) != 1 or flag(hi) != 0:
        return None
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        if flag(mid):
            lo = mid
        else:
            hi = mid
        if hi / lo - 1 < 1e-13:
            break
    return base, off, lo, hi


def two_sided(n, seed, n_out0, n_out1, fix_scale=False, th2=10.0, scale=None):
    """n clean pairs under two cameras with n_out0 gross outliers planted in obs1 and n_out1 others in obs2; returns (problem, idx0, idx1)"""
    p = two_camera(synth.make_sim3_problem(n, seed, outlier_frac=0.0, fix_scale=fix_scale))
    if scale is not None:
        p = with_scale(p, scale)
    rng = np.random.default_rng(100000 + seed)
    idx = rng.permutation(n)[:n_out0 + n_out1]
    p = plant_outliers(p, 0, idx[:n_out0], rng)
    p = plant_outliers(p, 1, idx[n_out0:], rng)
    p["th2"] = th2
    return p, idx[:n_out0], idx[n_out0:]


def survivor_case(oracle, n, n_out, side, seed0=7000, tries=20):
    """a problem of n pairs whose first pass drops exactly the n_out pairs planted on `side` (the oracle's zero flags are that set), so that n - n_out pairs reach the
    `>= 10` gate of Optimizer.cpp:1015: with 10 survivors the oracle goes on (nIn > 0 required), with 9 it returns 0.  Seeds from a fixed start, at most `tries`."""
    for seed in range(seed0 + 100 * n + 10 * n_out + side, seed0 + 100 * n + 10 * n_out + side + 2 * tries, 2):
        p, i0, i1 = two_sided(n, seed, 0 if side else n_out, n_out if side else 0)
        idx = i1 if side else i0
        _, inl, nin = oracle.sim3_optimize(*args(p))
        if not np.array_equal(np.flatnonzero(inl == 0), np.sort(idx)):
            continue
        if (n - n_out >= 10) != (nin > 0):
            continue
        return p, idx
    raise AssertionError(f"no seed leaves exactly {n - n_out} of {n} survivors (side {side})")


SWEEP_SIZES = (10, 11, 12, 14, 16, 23, 40, 64, 100, 150, 257, 300, 459, 700)
SWEEP_FRACS = (0.0, 0.1, 0.3)
SWEEP_TH2 = (7.0, 10.0, 16.0)


def sweep_cases():
    """4 x 14 x 3 = 168 seeded problems: (k, n, seed, outlier fraction, planted side, fix_scale, th2)"""
    k = 0
    for rep in range(4):
        for n in SWEEP_SIZES:
            for of in SWEEP_FRACS:
                yield k, n, 6000 + k, of, k % 2, bool((k // 2) % 2), SWEEP_TH2[(k + rep) % 3]
                k += 1


def sweep_problem(case):
    """the problem of one sweep case (two cameras, round(of n) gross outliers split between the sides) and the pair j to plant: a pair that is not a gross outlier"""
    k, n, seed, of, side, fix_scale, th2 = case
    n_out = int(round(of * n))
    p, i0, i1 = two_sided(n, seed, (n_out + 1) // 2, n_out // 2, fix_scale=fix_scale, th2=th2)
    clean = np.setdiff1d(np.arange(n), np.concatenate([i0, i1]))
    return p, int(clean[(7 * k) % clean.size])


@functools.lru_cache(maxsize=None)
def _sweep(oracle):
    out = []
    for case in sweep_cases():
        p, j = sweep_problem(case)
        out.append((case, p, j, plant_at_threshold(oracle, p, j, case[4], case[6])))
    return out


def sweep(oracle):
    """[(case, problem, j, plant_at_threshold result or None)] of the whole sweep, computed once per process and shared; nothing in it is modified by its users"""
    return _sweep(oracle)


def sweep_variants(p, j, side, pl, deltas):
    """(delta, problem) for lo (1 - delta) and hi (1 + delta) of every delta"""
    base, off, lo, hi = pl
    for d in deltas:
        for s in (lo * (1 - d), hi * (1 + d)):
            yield d, planted(p, j, side, base, off, s)
