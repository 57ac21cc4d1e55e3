"""The reduced camera system [S | b_schur] the DEVICE builds (ccm_ba_debug_partial_reduced: ba_linearize_pts(_e), ba_linearize_cams, ba_dinv and
whichever Schur kernel the shape selects) against the long-double reference of tests/ba_reference.py, entry by entry, at the accumulation bound

    |S_dev - S_ref| <= (n + C_DEVICE) 2^-53 |S|_acc        (and the same for b)

with n, |S|_acc from the reference and C_DEVICE = 4 x the constant measured for the f64 oracle on the CPU (ba_reference.C_ORACLE).  The block
pattern is compared exactly first; every case asserts through `sizes` / the profiling counters which kernels it reached.  The end-to-end parity
tests of test_ba_gpu.py cannot see a kernel that is subtly wrong (LM corrects itself); these can (tests/test_ba_reference_cpu.py shows the bound
rejecting one missing pair instance and one flipped Huber decision)."""
import numpy as np
import pytest

from ccm_slam_amd import optimizer, synth
from ccm_slam_amd._lib import K
from tests import ba_reference as ref
from tests.test_ba_structure_gpu import dev_array

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.HAVE_EXTENDED, reason="numpy.longdouble has no 64-bit mantissa on this platform")]
LD = ref.LD
ROW_MIN_BLOCKS, ROW_MAX_EDGES, TPB = 256, 1000, 256     # kRowMinBlocks, kRowMaxEdges, kTPB of the device code


def device_system(ctx, h, lam):
    """(blocks [nb, 6, 6], blk_i, blk_j (slots), slot_cam, b [Cp, 6], sizes, (diag launches, off / row launches)) of one hook call"""
    ctx.prof_enable(-1); ctx.prof_reset()
    red = h.partial_reduced(lam)
    n_diag, _ = ctx.prof_read(K["BA_SCHUR_DIAG"])
    n_off, _ = ctx.prof_read(K["BA_SCHUR_OFF"])
    ctx.prof_enable(-2)
    sz = h.debug_sizes()
    Cp, nb = sz["Cp"], sz["Cp"] + sz["nOff"]
    assert red.size == 36 * nb + 6 * Cp
    bi = dev_array(h, "blk_i", np.int32).astype(np.int64)
    bj = dev_array(h, "blk_j", np.int32).astype(np.int64)
    slot_cam = dev_array(h, "slot_cam", np.int32).astype(np.int64)
    assert bi.size == nb and bj.size == nb and slot_cam.size == Cp
    return red[:36 * nb].reshape(nb, 6, 6), bi, bj, slot_cam, red[36 * nb:].reshape(Cp, 6), sz, (n_diag, n_off)


def schur_path(sz, launches):
    """which implementation of launch_schur ran, from the sizes and the launch counts"""
    n_diag, n_off = launches
    if sz["nOff"] <= ROW_MIN_BLOCKS:
        assert n_diag == 1 and n_off == (1 if sz["nOff"] else 0) and sz["row_units_max"] == 0
        return "off4"
    if sz["row_units_max"] > 0:
        assert n_diag == 0 and n_off == 1 and sz["max_cam_edges"] <= ROW_MAX_EDGES
        return "row3"
    assert n_diag == 1 and n_off == 1      # a camera above kRowMaxEdges observations, or rows whose partial sums do not fit the row kernel's LDS plan
    return "off1"


def compare(dev, sys, lam, label=""):
    """pattern exactly, then every entry of every block and of b at the bound; structural promises of the kernels; returns the largest used share of the bound"""
    B, bi, bj, slot_cam, b, sz, _ = dev
    cams = sys["cams"]
    n_c = cams.size
    assert np.array_equal(np.sort(slot_cam), cams), label               # same free cameras
    r_of_slot = sys["cam_idx"][slot_cam]                                # device slot -> reference camera index
    # diagonal blocks first, one per slot, in slot order; then each off-diagonal pair once
    assert np.array_equal(bi[:n_c], np.arange(n_c)) and np.array_equal(bj[:n_c], np.arange(n_c)), label
    assert np.all(bi[n_c:] != bj[n_c:]), label
    ri, rj = r_of_slot[bi], r_of_slot[bj]
    lo, hi = np.minimum(ri, rj), np.maximum(ri, rj)
    dev_keys = lo * n_c + hi
    ref_keys = sys["blk_ij"][:, 0] * n_c + sys["blk_ij"][:, 1]
    assert np.unique(dev_keys).size == dev_keys.size, f"{label}: a block is stored twice"
    assert np.array_equal(np.sort(dev_keys), np.sort(ref_keys)), f"{label}: block pattern differs: missing {set(ref_keys) - set(dev_keys)}, spare {set(dev_keys) - set(ref_keys)}"
    order = np.argsort(ref_keys)
    k_ref = order[np.searchsorted(ref_keys[order], dev_keys)]
    flip = ri > rj                                                      # the device holds the (j, i) block: compare with the transpose
    S_ref = sys["S"][k_ref]; S_ref[flip] = np.swapaxes(S_ref[flip], 1, 2)
    bound = ref.bound_S(sys, ref.C_DEVICE)[k_ref]; bound[flip] = np.swapaxes(bound[flip], 1, 2)
    err = np.abs(B.astype(LD) - S_ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
    w = np.unravel_index(np.argmax(ratio), ratio.shape)
    worst_S = float(ratio[w])
    assert worst_S <= 1.0, (f"{label}: S block {w[0]} (cameras {cams[ri[w[0]]]}, {cams[rj[w[0]]]}) entry ({w[1]}, {w[2]}): device {B[w]!r} reference {float(S_ref[w])!r} "
                            f"|diff| {float(err[w]):.3e} bound {float(bound[w]):.3e} n {int(sys['S_n'][k_ref[w[0]]])}")
    b_ref = sys["b"][r_of_slot]; b_bound = ref.bound_b(sys, ref.C_DEVICE)[r_of_slot]
    eb = np.abs(b.astype(LD) - b_ref)
    rb = np.where(b_bound > 0, eb / np.where(b_bound > 0, b_bound, 1), np.where(eb > 0, np.inf, 0))
    wb = np.unravel_index(np.argmax(rb), rb.shape) if rb.size else None
    worst_b = float(rb[wb]) if rb.size else 0.0
    assert worst_b <= 1.0, (f"{label}: b of camera {cams[r_of_slot[wb[0]]]} entry {wb[1]}: device {b[wb]!r} reference {float(b_ref[wb])!r} |diff| {float(eb[wb]):.3e} "
                            f"bound {float(b_bound[wb]):.3e}")
    # what the kernels promise structurally: diagonal blocks bit-symmetric; the reference's S + lam I positive definite
    assert np.array_equal(B[:n_c], np.swapaxes(B[:n_c], 1, 2)), f"{label}: a diagonal block is not symmetric"
    np.linalg.cholesky(ref.dense(sys, lam).astype(np.float64))
    share = ref.wide_share(sys)
    assert share <= ref.WIDE_SHARE_CAP, (label, share)
    print(f"{label}: Cp {n_c} blocks {bi.size} used share of the bound S {worst_S:.3f} b {worst_b:.3f} cond(D) max {sys['condD'].max():.3g} widened {share:.4f}")
    return worst_S, worst_b


def compare_with_empty_blocks(dev, sys, lam, label):
    """a live handle keeps its block structure when edges leave: blocks the smaller problem does not have must be EXACTLY zero, the others compare as usual"""
    B, bi, bj, slot_cam, b, sz, launches = dev
    n_c = sys["cams"].size
    r = sys["cam_idx"][slot_cam]
    assert np.all(r >= 0)
    keys = np.minimum(r[bi], r[bj]) * n_c + np.maximum(r[bi], r[bj])
    ref_keys = sys["blk_ij"][:, 0] * n_c + sys["blk_ij"][:, 1]
    has = np.isin(keys, ref_keys)
    assert not np.any(B[~has]), f"{label}: a block without an active pair instance is not zero"
    compare((B[has], bi[has], bj[has], slot_cam, b, sz, launches), sys, lam, label)


def check(ctx, prob, lam_scale=1e-5, expect=None, label="", nranks=1, rank=0):
    sys0 = ref.reduced_system(prob, 1.0)
    lam = float(lam_scale * sys0["max_diag"])
    h = optimizer.BAHandle(ctx, prob, rank=rank, nranks=nranks)
    try:
        dev = device_system(ctx, h, lam)
        sz = dev[5]
        path = schur_path(sz, dev[6])
        if expect:
            assert path == expect, (label, path, sz)
        if nranks == 1:
            sys = ref.reduced_system(prob, lam)
        else:
            slot_pt = dev_array(h, "slot_pt", np.int32)
            own = slot_pt[sz["lp_begin"]:sz["lp_begin"] + sz["Lloc"]]
            assert own.size and np.all(np.diff(own) > 0)
            sys = ref.reduced_system(prob, lam, pt_lo=int(own[0]), pt_hi=int(own[-1]) + 1)
            assert np.array_equal(sys["pts"], own)
        # every rank lays out the GLOBAL block structure (the all-reduce sums buffers of one shape): blocks without an own pair instance are exact zeros
        (compare if nranks == 1 else compare_with_empty_blocks)(dev, sys, lam, label)
        return sz, path
    finally:
        h.close()


# ---- per-block kernels (<= 256 off-diagonal blocks) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(kfs_per_agent=2, n_points=80, seed=21, loop_len=40), dict(kfs_per_agent=3, n_points=80, seed=21, loop_len=40), dict(kfs_per_agent=12, n_points=500, seed=23)],
                         ids=["2cams_1free", "3cams", "12cams"])
def test_small_maps_diag_and_off4(ctx, kw):
    sz, _ = check(ctx, synth.make_ba_problem(n_agents=1, **kw), expect="off4", label=str(kw))
    assert sz["Cp"] == kw["kfs_per_agent"] - 1 and sz["n_chunk"] > 0


# ---- the row kernel, blocks longer than one work unit --------------------------------------------------------------------------------
@pytest.mark.parametrize("n_agents, kfs, n_points, mean_track, max_track", [(1, 48, 5800, 6.0, 30), (2, 60, 6000, 6.0, 30), (3, 60, 7000, 8.0, 40)],
                         ids=["47cams", "119cams", "179cams"])
def test_row_kernel_with_split_blocks(ctx, n_agents, kfs, n_points, mean_track, max_track):
    prob = synth.make_ba_problem(n_agents=n_agents, kfs_per_agent=kfs, n_points=n_points, mean_track=mean_track, max_track=max_track, seed=31)
    h = optimizer.BAHandle(ctx, prob)
    sz = h.debug_sizes()
    u0 = dev_array(h, "blk_unit0", np.int32)
    h.close()
    assert sz["Cp"] == n_agents * kfs - 1 and sz["row_units_max"] > 1
    assert np.diff(u0).max() >= 3, "no block is split over three work units"
    check(ctx, prob, expect="row3", label=f"{n_agents}x{kfs}")


# ---- both sides of kRowMaxEdges --------------------------------------------------------------------------------------------------------
def _one_busy_camera(n_obs, n_cam=61, n_shared=400, seed=5):
    """61 cameras (identity rotation) on a ring; 400 landmarks each seen by 6 consecutive cameras, so every free camera has 5 neighbours on either side
    (300 blocks > 256, at most 64 pair instances = one work unit per block, 10 units per row: inside the row kernel's LDS plan even beside 1000 observations);
    camera 1 also observes landmarks of its own, shared with the FIXED camera 0 only (no block), up to exactly n_obs observations."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = 458.654, 457.296, 367.215, 248.375
    ang = 2 * np.pi * np.arange(n_cam) / n_cam
    c = np.column_stack([np.cos(ang), np.sin(ang), rng.uniform(-0.3, 0.3, n_cam)])
    first = rng.integers(1, n_cam, n_shared)
    sh_cam = 1 + (first[:, None] - 1 + np.arange(6)[None]) % (n_cam - 1)            # cameras 1 .. 60, wrapping
    own = n_obs - int((sh_cam == 1).sum())
    n_pt = n_shared + own
    gt_pt = np.column_stack([rng.uniform(-3, 3, n_pt), rng.uniform(-2, 2, n_pt), rng.uniform(5, 9, n_pt)])
    e_pt = np.concatenate([np.repeat(np.arange(n_shared), 6), np.repeat(np.arange(n_shared, n_pt), 2)])
    e_cam = np.concatenate([sh_cam.ravel(), np.tile([0, 1], own)])
    order = np.lexsort((e_cam, e_pt))
    e_cam, e_pt = e_cam[order].astype(np.int32), e_pt[order].astype(np.int32)
    Xc = gt_pt[e_pt] - c[e_cam]
    obs = np.column_stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy]) + rng.normal(0, 1.0, (e_cam.size, 2))
    cam0 = np.zeros((n_cam, 7)); cam0[:, 3] = 1.0; cam0[:, 4:7] = -c + rng.normal(0, 0.02, (n_cam, 3))
    cam0[:, :3] = rng.normal(0, 0.004, (n_cam, 3)); cam0[:, :4] /= np.linalg.norm(cam0[:, :4], axis=1, keepdims=True)
    fixed = np.zeros(n_cam, np.uint8); fixed[0] = 1
    return {"n_cam": n_cam, "n_pt": n_pt, "n_edge": int(e_cam.size), "cam_qt": cam0.astype(np.float32).astype(np.float64), "cam_fixed": fixed,
            "cam_K": np.tile(np.array([fx, fy, cx, cy]), (n_cam, 1)), "pt_xyz": (gt_pt + rng.normal(0, 0.03, gt_pt.shape)).astype(np.float32).astype(np.float64),
            "e_cam": e_cam, "e_pt": e_pt, "e_obs": obs, "e_info": np.ones(e_cam.size), "e_level": np.zeros(e_cam.size, np.uint8),
            "huber_delta": float(np.sqrt(5.991))}


@pytest.mark.parametrize("n_obs, path", [(999, "row3"), (1000, "row3"), (1001, "off1")])
def test_camera_list_at_the_row_kernels_limit(ctx, n_obs, path):
    prob = _one_busy_camera(n_obs)
    assert np.bincount(prob["e_cam"]).max() == n_obs
    sz, _ = check(ctx, prob, expect=path, label=f"busy camera {n_obs}")
    assert sz["max_cam_edges"] == n_obs and sz["nOff"] == 300


# ---- a landmark at the chunked linearisation's limit ---------------------------------------------------------------------------------
def _one_long_track(n_track, n_cam=262, n_pt=420, seed=8):
    """262 cameras on a line looking the same way; landmark 0 is observed by exactly n_track of them, every other landmark by 5 neighbouring ones."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = 458.654, 457.296, 367.215, 248.375
    c = np.column_stack([np.linspace(-2.0, 2.0, n_cam), rng.uniform(-0.2, 0.2, n_cam), rng.uniform(-0.2, 0.2, n_cam)])
    gt_pt = np.column_stack([rng.uniform(-2.5, 2.5, n_pt), rng.uniform(-1.5, 1.5, n_pt), rng.uniform(5, 9, n_pt)])
    gt_pt[0] = [0.1, -0.2, 7.0]
    first = rng.integers(0, n_cam - 5, n_pt)
    e_pt = np.concatenate([np.zeros(n_track, np.int64), np.repeat(np.arange(1, n_pt), 5)])
    e_cam = np.concatenate([np.arange(n_track), (first[1:, None] + np.arange(5)[None]).ravel()])
    Xc = gt_pt[e_pt] - c[e_cam]
    obs = np.column_stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy]) + rng.normal(0, 1.0, (e_cam.size, 2))
    cam0 = np.zeros((n_cam, 7)); cam0[:, 3] = 1.0; cam0[:, 4:7] = -c + rng.normal(0, 0.01, (n_cam, 3))
    cam0[:, :3] = rng.normal(0, 0.002, (n_cam, 3)); cam0[:, :4] /= np.linalg.norm(cam0[:, :4], axis=1, keepdims=True)
    fixed = np.zeros(n_cam, np.uint8); fixed[0] = 1
    return {"n_cam": n_cam, "n_pt": n_pt, "n_edge": int(e_cam.size), "cam_qt": cam0.astype(np.float32).astype(np.float64), "cam_fixed": fixed,
            "cam_K": np.tile(np.array([fx, fy, cx, cy]), (n_cam, 1)), "pt_xyz": (gt_pt + rng.normal(0, 0.03, gt_pt.shape)).astype(np.float32).astype(np.float64),
            "e_cam": e_cam.astype(np.int32), "e_pt": e_pt.astype(np.int32), "e_obs": obs, "e_info": np.ones(e_cam.size), "e_level": np.zeros(e_cam.size, np.uint8),
            "huber_delta": float(np.sqrt(5.991))}


@pytest.mark.parametrize("n_track", [256, 257])
def test_landmark_at_the_chunked_linearisations_limit(ctx, n_track):
    """256 observations: ba_linearize_pts_e (chunks of <= 256 observations); 257: the thread-per-landmark ba_linearize_pts"""
    prob = _one_long_track(n_track)
    assert np.bincount(prob["e_pt"]).max() == n_track
    sz, _ = check(ctx, prob, label=f"track {n_track}")
    assert (sz["n_chunk"] > 0) == (n_track <= TPB), sz


# ---- structure edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fixed", [0, 3, 8])
def test_fixed_cameras_at_the_tail(ctx, n_fixed):
    """n_fixed from 0 to 40 % of a 20-camera window, fixed at the tail: landmarks seen by fixed cameras only plus one free one, by one free camera only"""
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=20, n_points=900, n_fixed=n_fixed, fixed_mode="tail", seed=40 + n_fixed)
    sz, _ = check(ctx, prob, label=f"tail {n_fixed}")
    assert sz["Cp"] == 20 - n_fixed


def test_cameras_without_an_off_diagonal_block(ctx):
    """three maps that share no landmark, each a single free camera among fixed ones: every row of S is its diagonal block alone"""
    prob = synth.make_ba_problem(n_agents=3, kfs_per_agent=8, loop_len=40, n_points=400, cross_frac=0.0, n_fixed=7, fixed_mode="tail", seed=50)
    h = optimizer.BAHandle(ctx, prob)
    bi, bj = dev_array(h, "blk_i", np.int32), dev_array(h, "blk_j", np.int32)
    Cp = h.debug_sizes()["Cp"]
    h.close()
    assert Cp == 3 and not np.any(bi != bj)
    check(ctx, prob, expect="off4", label="no off-diagonal block")


# ---- deactivated edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [0.0, 0.3, 1.0])
def test_edge_levels_at_create_and_on_a_live_handle(ctx, share):
    """`share` of camera 5's observations at level 1: given at create, and through ccm_ba_set_edge_levels on a live handle (zeroed informations,
    ba_deactivate_edges + ba_refresh_cam_info), then back to all-zero: every time the reference of the problem with exactly those edges."""
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=14, n_points=600, seed=60)
    mine = np.flatnonzero(prob["e_cam"] == 5)
    lvl = np.zeros(prob["n_edge"], np.uint8)
    lvl[mine[:int(round(share * mine.size))]] = 1
    p1 = dict(prob); p1["e_level"] = lvl
    if share < 1.0:     # (with every edge of the camera gone it is no vertex of a problem created that way; the live handle keeps it, see below)
        check(ctx, p1, label=f"levels {share} at create")
    lam = float(1e-5 * ref.reduced_system(prob, 1.0)["max_diag"])
    h = optimizer.BAHandle(ctx, prob)
    try:
        h.set_edge_levels(lvl, prob["huber_delta"])
        dev = device_system(ctx, h, lam)
        sys = ref.reduced_system(p1, lam)
        if share == 1.0:
            # the live handle still carries camera 5 as a vertex with an all-zero row; the reference has no such camera
            slot = int(np.flatnonzero(dev[3] == 5)[0])
            B, bi, bj = dev[0], dev[1], dev[2]
            assert not np.any(B[(bi == slot) | (bj == slot)]) and not np.any(dev[4][slot])
            dev_keep = (bi != slot) & (bj != slot)
            remap = np.cumsum(np.arange(dev[3].size) != slot) - 1
            dev2 = (B[dev_keep], remap[bi[dev_keep]], remap[bj[dev_keep]], np.delete(dev[3], slot), np.delete(dev[4], slot, 0), dev[5], dev[6])
            compare_with_empty_blocks(dev2, sys, lam, "levels 1.0 live")
        else:
            compare_with_empty_blocks(dev, sys, lam, f"levels {share} live")
        h.set_edge_levels(np.zeros(prob["n_edge"], np.uint8), prob["huber_delta"])
        compare(device_system(ctx, h, lam), ref.reduced_system(prob, lam), lam, f"levels {share} back to zero")
    finally:
        h.close()


# ---- the Huber threshold ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rel", [-2.0 ** -30, 0.0, 2.0 ** -30], ids=["below", "on", "above"])
def test_residual_planted_at_the_huber_threshold(ctx, rel):
    """e2 = dsqr (1 + rel), exactly representable (ba_reference.planted_huber_problem), dsqr the f32-rounded delta^2 of sqrt(5.991) as f32"""
    prob, k = ref.planted_huber_problem(rel)
    check(ctx, prob, lam_scale=1e-4, expect="off4", label=f"huber rel {rel:+.1e}")


def test_no_robust_kernel(ctx):
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=12, n_points=500, seed=23, huber_delta=0.0)
    check(ctx, prob, expect="off4", label="huber_delta 0")


# ---- damping ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-7, 1e-4, 1e-1, 1e2])
def test_damping_over_nine_decades(ctx, scale):
    """ba_dinv at lambda = scale x the largest diagonal entry, on a row-kernel map"""
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=40, n_points=3000, seed=70)
    check(ctx, prob, lam_scale=scale, expect="row3", label=f"lambda {scale:g}")


# ---- one rank's part of a sharded build ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks", [2, 3])
def test_each_ranks_partial_system(ctx, nranks):
    """every rank's buffer against the reference restricted to that rank's landmarks (lp_begin, Lloc), not only their sum"""
    prob = synth.make_ba_problem(n_agents=2, kfs_per_agent=12, n_points=900, seed=77)
    for r in range(nranks):
        check(ctx, prob, nranks=nranks, rank=r, label=f"rank {r} of {nranks}")


# ---- the double-buffered state ---------------------------------------------------------------------------------------------------------
def test_after_a_run_and_after_push_run_pop(ctx):
    """after run(2) the estimate lives in the other buffer: the hook must linearise THERE (reference at the downloaded state); after push / run / pop
    it must be back at the pushed state, bit for bit"""
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=30, n_points=1500, seed=80)
    lam = float(1e-5 * ref.reduced_system(prob, 1.0)["max_diag"])
    h = optimizer.BAHandle(ctx, prob)
    try:
        st = h.run(2)
        assert st.iters_done == 2
        cam, pts, _, _ = h.download()
        assert np.abs(cam - prob["cam_qt"]).max() > 1e-6
        dev = device_system(ctx, h, lam)
        compare(dev, ref.reduced_system(prob, lam, cam_qt=cam, pt_xyz=pts), lam, "after run(2)")
        h.push_state()
        h.run(3)
        h.pop_state()
        dev2 = device_system(ctx, h, lam)
        assert np.array_equal(dev[0], dev2[0]) and np.array_equal(dev[4], dev2[4])
    finally:
        h.close()
