"""CPU: how sharp are the observables of Optimizer::OptimizeSim3 (Optimizer.cpp:861-1056: per pair `chi2 > th2` on either edge after each pass, the inlier count,
the optimised S12) as a function of the reference's OWN arithmetic?  As in tests/test_poseopt_threshold_cpu.py the oracle's restatement is compiled twice from the
same source — as the reference is built (-O2, no FMA contraction: liboracle.so) and with -O3 -march=native (FMA contraction allowed: liboracle_fast.so, a legal
compilation of the same C++) — and both run on the sweep of tests/sim3_opt_cases.py: 168 problems (10 .. 700 pairs, two cameras, gross outliers on both sides,
th2 7 / 10 / 16, free and fixed scale) as generated, and the 151 of them on which plant_at_threshold succeeds again with one residual planted at a relative
distance delta from the point where the plain build's decision for that pair flips (302 calls per delta).

Measured here (the figures that tests/test_sim3_gpu.py and DESIGN.md quote):
  flags / nIn differ in 0 of 168 calls as generated and in 0 / 0 / 1 / 17 / 99 of 302 calls at delta 1e-4 / 1e-5 / 1e-6 / 1e-7 / 1e-8
    => the device must agree at 1e-4 and 1e-5 (one decade above the largest delta at which the reference disagrees with itself), and is counted at 1e-6 / 1e-7
       against twice these shares (0.33 % and 5.6 %; sim3_opt_cases.share_cap);
  Sim3 estimates, identical flags and nIn >= 16: at most 1.01e-5 (one problem of 700 pairs planted at 1e-4 / 1e-5; 4.2e-7 over all other cases)
    => sim3_opt_cases.REF_SPREAD, device tolerance 4 x that.
"""
import numpy as np

import sim3_opt_cases as sc


def test_flags_and_estimate_between_two_builds_of_the_reference(oracle_lib):
    fast = oracle_lib.fast_lib()
    deltas = sc.MUST_DELTAS + sc.COUNTED_DELTAS + (1e-8,)
    diff = {d: 0 for d in deltas}
    calls = {d: 0 for d in deltas}
    spread = 0.0
    wider = [0]   # differing calls in which more than pair j's flag and one count differ

    def both(p, j=None):
        want = oracle_lib.sim3_optimize(*sc.args(p))
        got = sc.fast_sim3(fast, p)
        same = want[2] == got[2] and np.array_equal(want[1], got[1])
        if not same and j is not None:   # the rule the GPU test applies to the device holds between the reference's own builds
            assert sc.planted_pair_differs(j, got, want), (j, np.flatnonzero(got[1] != want[1]), got[2], want[2])
            wider[0] += 0 if sc.only_planted_pair(j, got, want) else 1
        return same, (float(np.abs(want[0] - got[0]).max()) if same and want[2] >= sc.MIN_INLIERS_FOR_ESTIMATE else 0.0)

    n_planted = 0
    for case, p, j, pl in sc.sweep(oracle_lib):
        same, d_est = both(p)
        assert same, ("as generated", case)
        spread = max(spread, d_est)
        if pl is None:
            continue
        n_planted += 1
        for d, q in sc.sweep_variants(p, j, case[4], pl, deltas):
            same, d_est = both(q, j)
            calls[d] += 1
            diff[d] += 0 if same else 1
            if d in sc.MUST_DELTAS:
                spread = max(spread, d_est)
    share = {d: diff[d] / calls[d] for d in deltas}
    print(f"planted {n_planted}, calls per delta {calls[1e-8]}, builds differ in {diff}; of these {wider[0]} in more than the planted pair; estimate spread (must cases, same flags, nIn >= 16) {spread:.3e}")
    assert n_planted >= 120 and sum(calls[d] for d in sc.MUST_DELTAS) >= 400, (n_planted, calls)
    for d in sc.MUST_DELTAS:
        assert diff[d] == 0, diff
    assert diff[1e-8] > 0, diff   # (if this ever fails the two builds have become identical: the yardstick is gone, not the sensitivity)
    # the literals that the GPU test takes from here still describe this reference: its own shares stay under the caps derived from them, its own spread under the tolerance
    for d in sc.COUNTED_DELTAS:
        assert share[d] <= sc.share_cap(d), (d, share[d], sc.share_cap(d))
    assert spread <= sc.EST_TOL, spread


def test_the_new_cases_hold_on_the_oracle_alone(oracle_lib):
    """survivor_case finds its problems within its 20 seeds, with 10 survivors the estimate moves, with 9 it stays; the staging sizes are the host's"""
    for n, n_out in ((14, 4), (14, 5), (30, 20), (30, 21), (10, 0), (10, 1)):
        for side in (0, 1):
            p, idx = sc.survivor_case(oracle_lib, n, n_out, side)
            s, inl, nin = oracle_lib.sim3_optimize(*sc.args(p))
            assert np.array_equal(np.flatnonzero(inl == 0), np.sort(idx))
            if n - n_out >= 10:
                assert nin == 10 and not np.array_equal(s, p["sim3"])
            else:
                assert nin == 0 and np.array_equal(s, p["sim3"])
    assert sc.STAGING_EDGES == (458, 459, 1136, 1137)
    assert sc.lds_full(458) <= 64 * 1024 < sc.lds_full(459)
    assert 5904 + 130 * 1136 <= 150 * 1024 < 5904 + 130 * 1137


def test_the_staging_sizes_are_those_of_the_host_code():
    """The launch shapes cannot be told apart through the call (a staged and an unstaged run of one problem return the same bits, and the runtime launches any
    dynamic LDS size the CU holds, whatever limit was requested), so the figures that sim3_opt_cases.STAGING_EDGES is derived from are read from the host code:
    head doubles, bytes per pair, and ONE limit that both decides on staging and is requested for the kernel."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ccm_slam_amd", "csrc")
    red = open(os.path.join(csrc, "block_red.h")).read()
    src = open(os.path.join(csrc, "sim3opt.hip")).read()

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]
    n_waves = int(one(r"constexpr int kNW = (\d+);", red))
    one(r"constexpr int kRedDoubles = 2 \* kNW \* 64;", red)
    pert = one(r"constexpr int kPertDoubles = (\d+) \* (\d+);", src)
    head = (2 * n_waves * 64 + int(pert[0]) * int(pert[1])) * 8
    one(r"const size_t lds_head = \(kRedDoubles \+ kPertDoubles\) \* sizeof\(double\);", src)
    pair = one(r"const size_t lds_full = lds_head \+ (\d+) \* \(size_t\)n \* sizeof\(double\) \+ (\d+) \* \(size_t\)n \+ (\d+);", src)
    assert head == sc.LDS_HEAD and int(pair[0]) * 8 + int(pair[1]) == sc.LDS_PER_PAIR and head + int(pair[2]) == sc.lds_full(0) == 5904
    staged_limit = int(one(r"const int use_lds = lds_full <= (\d+) \* 1024;", src))
    plain_limit = int(one(r"if \(lds_bytes > (\d+) \* 1024\) \{", src))
    requested = int(one(r"CCM_LDS_ATTR\(ctx, CCM_LDS_SIM3OPT, sim3opt_kernel, (\d+) \* 1024\);", src))
    assert staged_limit == requested == 150 and plain_limit == 64     # never stage more than was requested for the kernel
    assert sc.N_PLAIN_MAX == (plain_limit * 1024 - 5904) // 130 and sc.N_LDS_MAX == (staged_limit * 1024 - 5904) // 130


def test_case_builders_keep_the_problem_consistent():
    from ccm_slam_amd import synth
    p0 = synth.make_sim3_problem(40, 11, outlier_frac=0.0, fix_scale=True)
    p = sc.two_camera(p0)
    # the normalised image points of keyframe 2 are those of the generated problem, to f32 rounding of a ~700 px coordinate (2^-15 px)
    x0 = (p0["obs2"] - p0["K2"][2:]) / p0["K2"][:2]
    x = (p["obs2"] - p["K2"][2:]) / p["K2"][:2]
    assert np.abs(x - x0).max() < 2.0 ** -14 / 435.0 and not np.array_equal(p["K1"], p["K2"])
    assert np.array_equal(p["obs1"], p0["obs1"])
    # with_scale: the truth at scale s maps the shrunk P2c onto P1c as the truth at scale 1 mapped the original (to the maps' 0.01 m disagreement)
    q = sc.with_scale(p, 0.8)
    assert q["sim3"][7] == 0.8 and np.array_equal(q["sim3"][:7], p["sim3"][:7])
    a = sc.sim3_project(p["gt_sim3"], p["P2c"], p["K1"], False)
    b = sc.sim3_project(q["gt_sim3"], q["P2c"], q["K1"], False)
    assert np.abs(a - b).max() < 1e-3
    # plant_outliers: 30 .. 60 px on the chosen pairs of the chosen side only
    rng = np.random.default_rng(0)
    r = sc.plant_outliers(p, 1, [3, 7], rng)
    d = np.abs(r["obs2"] - p["obs2"])
    assert np.array_equal(np.flatnonzero(d.max(1) > 0), [3, 7]) and d[[3, 7]].min() > 29.9 and d.max() < 60.1
    assert np.array_equal(r["obs1"], p["obs1"])
