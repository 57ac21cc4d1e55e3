"""GPU: ccm_fuse_pose_eval equals the host evaluator (csrc/fuse_math.h under g++) bit for bit, and the reference's own ORBmatcher::Fuse where
oracle/_ref/libmatcher_ref.so was built on this machine, at every size where the kernel takes another path: one pair, no job, empty jobs between others, tiles of
256 pairs that are full, one short and one over, waves that are full, one short and one over, job lists whose tiles belong to different keyframes, windows that a
lane walks alone and windows the wave takes (the switch is 64 features in the window's cells), many small jobs, a keyframe without features.  Every comparison is
exact."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import oracle
import tests.test_ref_matcher as trm
from ccm_slam_amd import fuse_pose as fp, fuse_sim3 as fs, synth
from fuse_pose_cases import CALLS, CURRENT, DISC_SIZES, DISC_WHOLE, N_KF, assert_reference_scene, disc, disc_gate_counts, fan_out_scene, planted, ref_fuse
from fuse_sim3_cases import same_as_reference
from test_fuse_pose_cpu import N_PREDICTED, bad_argument_cases, call_raw, each_job_equals_itself_alone, mirror_scene, walk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    o = oracle.OrbOracle(1000)
    out = [o.extract(synth.gen_image(1000, t)) for t in (0, 1)]
    o.close()
    return out


@pytest.fixture(scope="module")
def scene(frames):
    return fan_out_scene(frames)


def sin_jobs(info):
    """the SearchInNeighbors shape: the 12 calls of the fan-out (8 keyframes) on the current keyframe's 2 500 points, then the current keyframe on 6 000 points"""
    return [(k, 0, info["n1"]) for k in CALLS] + [(CURRENT, 1500, 6000)]


@pytest.fixture(scope="module")
def sin_scene(scene):
    sc, info = scene
    s = sc.subset(jobs=sin_jobs(info))
    return s, fp.fuse_pose_eval_host(s, want_uv=True)


def same(got, want, tag):
    assert np.array_equal(got["table"], want["table"]), tag
    assert np.array_equal(got["n_valid"], want["n_valid"]) and np.array_equal(got["n_hit"], want["n_hit"]), tag
    if "uv" in got:
        assert np.array_equal(got["uv"].view(np.uint32), want["uv"].view(np.uint32)), tag
    st = fs.unpack_table(got["table"])["status"]
    off = got["job_off"]
    for j in range(got["n_valid"].size):      # the counters against the table
        part = st[off[j]:off[j + 1]]
        assert got["n_valid"][j] == (part >= 4).sum() and got["n_hit"][j] == (part == 7).sum(), (tag, j)


def both(ctx, s, tag, want_uv=True):
    got = fp.fuse_pose_eval(ctx, s, want_uv=want_uv)
    want = fp.fuse_pose_eval_host(s, want_uv=want_uv)
    same(got, want, tag)
    return got


def test_edge_shapes(ctx, scene):
    sc = scene[0]
    for kfs, P, jobs in (([0], 41, [(0, 40, 1)]), ([0], 41, []), ([], 0, []), ([], 7, []), ([0, 5], 300, [(0, 40, 70), (1, 5, 0), (1, 100, 130)]),
                         ([0, 5], 300, [(1, 300, 0)]), ([3], 0, [(0, 0, 0)])):
        got = both(ctx, sc.subset(kfs, P, jobs), (kfs, P, jobs))
        assert got["table"].size == sum(j[2] for j in jobs) and got["n_valid"].size == len(jobs)
    pl = planted()
    ps = pl.scene().subset([0], None, [(0, 0, len(pl.pts))])          # planted keyframe 0 has no features
    got = both(ctx, ps, "no features")
    assert got["n_hit"][0] == 0 and got["n_valid"][0] > 0


def test_tile_and_wave_edges(ctx, scene, sin_scene):
    sc = scene[0]
    s, want = sin_scene
    for J in (1, 2, 3):
        for n in (63, 64, 65, 255, 256, 257):
            jobs = [(CALLS[j], 40, n) for j in range(J)]          # (the scene's first 40 points lie behind the camera)
            got = both(ctx, sc.subset(jobs=jobs), (J, n))
            for j in range(J):
                assert np.array_equal(fp.job_rows(got, j), fp.job_rows(want, j)[40:40 + n])
            assert got["n_hit"].min() > 0


def test_jobs_of_different_sizes_on_different_keyframes_equal_each_job_alone(ctx, scene):
    """a wrong tile -> job map shows here: 1, 257, 0, 64 and 300 pairs on keyframes 2, 0, 1, 0, 2"""
    sc = scene[0]
    s = sc.subset(jobs=[(2, 50, 1), (0, 40, 257), (1, 0, 0), (0, 200, 64), (2, 100, 300)])
    got = both(ctx, s, "mixed sizes")
    each_job_equals_itself_alone(s, got, lambda one: fp.fuse_pose_eval(ctx, one, want_uv=True))
    assert got["n_hit"][[1, 3, 4]].min() > 10


def test_one_keyframe_in_two_jobs(ctx, scene):
    sc = scene[0]
    s = sc.subset(jobs=[(5, 0, 700), (5, 0, 700), (5, 300, 700), (1, 0, 10)])
    got = both(ctx, s, "one keyframe, three jobs")
    assert np.array_equal(fp.job_rows(got, 0), fp.job_rows(got, 1)) and np.array_equal(fp.job_rows(got, 0)[300:], fp.job_rows(got, 2)[:400])
    assert got["n_hit"][0] == got["n_hit"][1] > 100


def test_search_in_neighbors_shape_equals_the_host_evaluator_and_the_reference(ctx, frames, scene, sin_scene):
    sc, info = scene
    s, want = sin_scene
    got = fp.fuse_pose_eval(ctx, s, want_uv=True)
    same(got, want, "with uv")
    bare = fp.fuse_pose_eval(ctx, s)
    assert "uv" not in bare
    same(bare, want, "without uv")
    if os.path.exists(trm.LIB):
        rlib = C.CDLL(trm.LIB)
        refs = [ref_fuse(rlib, frames, sc, info, k) for k in range(N_KF)]
        assert_reference_scene(refs, frames, info, 3.0)
        t = fs.unpack_table(got["table"])
        for j, (k, p0, n) in enumerate(s.jobs):
            ref = refs[k] if p0 == 0 and n == info["n1"] else ref_fuse(rlib, frames, sc, info, k, pts=np.arange(p0, p0 + n))
            same_as_reference({m: fp.job_rows(dict(table=a, job_off=got["job_off"]), j) for m, a in t.items()}, fp.job_rows(got, j, "uv"), ref, f"job {j}")


def test_three_hundred_small_jobs(ctx, scene):
    sc = scene[0]
    s = sc.subset(jobs=[(j % N_KF, 30 + 7 * j, 40) for j in range(300)])
    got = both(ctx, s, "J = 300")
    assert len(set(got["n_hit"].tolist())) > 5 and got["n_hit"].max() > 15


def test_planted_boundaries(ctx):
    pl = planted()
    sc = pl.scene()
    got = both(ctx, sc, "planted")
    pl.check(got["table"], "device")
    both(ctx, pl.scene(inv_sigma2=np.zeros(8, np.float32)), "planted, zero inv_level_sigma2")


def test_windows_on_both_sides_of_the_wave_switch(ctx):
    pl = disc()
    sc = pl.scene()
    want = fp.fuse_pose_eval_host(sc, want_uv=True, want_cand=True)
    nc = want["n_cand"].reshape(sc.K, sc.P)
    # from level DISC_WHOLE on the window holds the whole disc, so its cells hold every feature of the keyframe: 0, 1, 60 and 64 features stay with the lane,
    # 65, 70 and 300 go to the wave
    for lvl in range(DISC_WHOLE, 8):
        assert nc[:, lvl].tolist() == list(DISC_SIZES)
    assert any(n <= 64 for n in DISC_SIZES[2:]) and any(64 < n <= 70 for n in DISC_SIZES) and nc.max() > 256
    for k, n in enumerate(DISC_SIZES):
        if n >= 60:
            ok, out = disc_gate_counts(pl, k, DISC_WHOLE)
            assert ok > 0 and out > 0, (n, ok, out)      # candidates on both sides of the chi-square gate in that window
    st = fs.unpack_table(want["table"])["status"]
    assert {4, 5, 6, 7} <= set(st.tolist())
    same(fp.fuse_pose_eval(ctx, sc, want_uv=True), want, "disc")


def test_repeated_calls_and_bad_arguments_on_one_context(ctx, scene, sin_scene):
    sc = scene[0]
    s, want = sin_scene
    small = sc.subset([1, 2], 300, [(1, 0, 300), (0, 100, 77)])
    wsmall = fp.fuse_pose_eval_host(small, want_uv=True)
    for rep in range(3):
        same(fp.fuse_pose_eval(ctx, s, want_uv=rep != 1), want, f"repeat {rep}")
        same(fp.fuse_pose_eval(ctx, small, want_uv=True), wsmall, f"small {rep}")
    for name, b in bad_argument_cases():
        assert call_raw(fp._dev().ccm_fuse_pose_eval, b, (ctx.handle,)) == -1, name     # CCM_E_ARG
    same(fp.fuse_pose_eval(ctx, small, want_uv=True), wsmall, "after the refusals")


def test_two_contexts_on_two_threads(scene):
    from ccm_slam_amd._lib import Context
    sc = scene[0]
    subs = [sc.subset([0, 2, 4], 1500, [(0, 0, 1500), (2, 100, 900), (1, 0, 1500)]), sc.subset([1, 3, 5, 7], 2500, [(k, 0, 2500) for k in (3, 0, 2, 1)])]
    wants = [fp.fuse_pose_eval_host(s, want_uv=True) for s in subs]
    errs = []

    def run(j):
        try:
            c = Context(0)
            try:
                for _ in range(4):
                    same(fp.fuse_pose_eval(c, subs[j], want_uv=True), wants[j], f"thread {j}")
            finally:
                c.close()
        except BaseException as e:   # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=run, args=(j,)) for j in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs


def test_mirror_on_the_device_through_the_fan_out_and_the_current_keyframe(ctx, frames, scene):
    """the CPU file's walk on a batch evaluated on the device; without the reference's library on this machine, against the mirror on the host evaluator"""
    sc, info = scene
    ms = mirror_scene(sc, info)
    P = info["n1"]
    dev = fp.SearchInNeighborsBatch(ctx, ms, CALLS, CURRENT, P)
    host = fp.SearchInNeighborsBatch(None, ms, CALLS, CURRENT, P)
    try:
        assert np.array_equal(dev.table()["table"], host.table()["table"]) and np.array_equal(dev.table()["n_hit"], host.table()["n_hit"])
        if os.path.exists(trm.LIB):
            walk(dev, sc, info, frames, C.CDLL(trm.LIB), dev.table()["calls"])
        else:
            rng = np.random.default_rng(5)
            kdesc = frames[0][1]
            skip = np.zeros(P, np.uint8); now = sc.pt_desc.reshape(-1, 32)[:P].copy()
            for c in range(len(CALLS)):
                a, b = dev.resolve(c, skip, now), host.resolve(c, skip, now)
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and dev.n_reeval() == host.n_reeval()
                fused = np.flatnonzero(a[1] >= 0)
                now[fused[0::3]] = kdesc[a[1][fused[0::3]]]
                skip[fused[1::3]] = 1; skip[rng.choice(P, 15, replace=False)] = 1
            assert host.n_reeval() > 100
            cand = rng.permutation(info["n2"])[:1560]
            slot = np.where(cand < N_PREDICTED, cand, -1).astype(np.int32)
            g = P + cand
            take = lambda a, w: a.reshape(-1, w)[g]
            desc_now = take(sc.pt_desc, 32).copy(); desc_now[::7] = kdesc[:desc_now[::7].shape[0]]
            fresh = (take(sc.pos, 3), take(sc.normal, 3), take(sc.min_dist, 1), take(sc.max_dist, 1), desc_now)
            a, b = dev.resolve_current(slot, None, desc_now, fresh), host.resolve_current(slot, None, desc_now, fresh)
            assert a[0] == b[0] > 100 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
            assert dev.n_reeval() == host.n_reeval() and dev.n_unpredicted() == host.n_unpredicted() >= 20
    finally:
        dev.close(); host.close()
