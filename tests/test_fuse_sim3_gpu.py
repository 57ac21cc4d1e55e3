"""GPU: ccm_fuse_sim3_eval equals the host evaluator (csrc/fuse_math.h under g++) bit for bit, and the reference's own ORBmatcher::Fuse where
oracle/_ref/libmatcher_ref.so was built on this machine, at every size where the kernel takes another path: one pair, no pair, tiles of 256 points that are
full, one short and one over, waves that are full, one short and one over, windows that a lane walks alone and windows the wave takes (the switch is 64 features
in the window's cells), many keyframes, a keyframe without features.  Every comparison is exact."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import oracle
import tests.test_ref_matcher as trm
from ccm_slam_amd import fuse_sim3 as fs, synth
from fuse_sim3_cases import DISC_SIZES, assert_reference_scene, disc, planted, ref_fuse, same_as_reference, scene_from_frames
from test_fuse_sim3_cpu import KINDS, bad_argument_cases, huge_product_case, walk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames():
    o = oracle.OrbOracle(1000)
    out = [o.extract(synth.gen_image(1000, t)) for t in (0, 1)]
    o.close()
    return out


@pytest.fixture(scope="module")
def mixed(frames):
    sc, s, S16, which = scene_from_frames(frames, KINDS)
    return sc, s, S16, which, fs.fuse_sim3_eval_host(sc, want_uv=True)


def same(got, want, tag):
    assert np.array_equal(got["table"], want["table"]), tag
    assert np.array_equal(got["n_valid"], want["n_valid"]) and np.array_equal(got["n_hit"], want["n_hit"]), tag
    if "uv" in got:
        assert np.array_equal(got["uv"].view(np.uint32), want["uv"].view(np.uint32)), tag
    t = fs.unpack_table(got["table"])
    assert np.array_equal(got["n_valid"], (t["status"] >= 4).sum(1)) and np.array_equal(got["n_hit"], (t["status"] == 7).sum(1)), tag


def test_one_pair_no_pair_and_a_keyframe_without_features(ctx, mixed):
    sc = mixed[0]
    for kfs, P in (([0], 1), ([0], 0), ([], 7), ([], 0), ([0, 5], 1)):
        sub = sc.subset(kfs, P)
        got = fs.fuse_sim3_eval(ctx, sub, want_uv=True)
        assert got["table"].shape == (len(kfs), P)
        same(got, fs.fuse_sim3_eval_host(sub, want_uv=True), (kfs, P))
    pl = planted()
    ps = pl.scene().subset([0], None)          # planted keyframe 0 has no features
    got = fs.fuse_sim3_eval(ctx, ps, want_uv=True)
    same(got, fs.fuse_sim3_eval_host(ps, want_uv=True), "no features")
    assert got["n_hit"][0] == 0 and got["n_valid"][0] > 0


def test_tile_and_wave_edges_on_near_keyframes(ctx, mixed):
    sc, _, _, _, want = mixed
    near = [k for k, c in enumerate(KINDS) if c == "n"]
    for K in (1, 2, 3):
        for P in (63, 64, 65, 255, 256, 257):
            sub = sc.subset(near[:K], P)
            got = fs.fuse_sim3_eval(ctx, sub, want_uv=True)
            same(got, fs.fuse_sim3_eval_host(sub, want_uv=True), (K, P))
            assert np.array_equal(got["table"], want["table"][near[:K], :P])
            assert got["n_hit"].min() > 0 and got["n_valid"].max() <= P - 40      # the scene's first 40 points lie behind the camera


def test_mixed_scene_equals_the_host_evaluator_and_the_reference(ctx, frames, mixed):
    sc, s, S16, which, want = mixed
    got = fs.fuse_sim3_eval(ctx, sc, want_uv=True)
    same(got, want, "with uv")
    bare = fs.fuse_sim3_eval(ctx, sc)
    assert "uv" not in bare
    same(bare, want, "without uv")
    if os.path.exists(trm.LIB):
        rlib = C.CDLL(trm.LIB)
        refs = [ref_fuse(rlib, frames, s, S16, which, k) for k in range(sc.K)]
        assert_reference_scene(refs, KINDS)
        t = fs.unpack_table(got["table"])
        for k in range(sc.K):
            same_as_reference({n: a[k] for n, a in t.items()}, got["uv"][k], refs[k], f"keyframe {k}")


def test_three_hundred_keyframes(ctx, frames):
    kinds = "".join("nf"[(k // 2) % 2] for k in range(300))
    sc = scene_from_frames(frames, kinds, seed=9, n_pts=40, first=30)[0]      # 10 points behind the camera, 30 in front
    want = fs.fuse_sim3_eval_host(sc, want_uv=True)
    assert len(set(want["n_hit"].tolist())) > 5 and want["n_hit"].max() > 20
    same(fs.fuse_sim3_eval(ctx, sc, want_uv=True), want, "K = 300")


def test_planted_boundaries(ctx):
    pl = planted()
    sc = pl.scene()
    got = fs.fuse_sim3_eval(ctx, sc, want_uv=True)
    pl.check(got["table"], "device")
    same(got, fs.fuse_sim3_eval_host(sc, want_uv=True), "planted")


def test_windows_on_both_sides_of_the_wave_switch(ctx):
    pl = disc()
    sc = pl.scene()
    want = fs.fuse_sim3_eval_host(sc, want_uv=True, want_cand=True)
    # the cells of the level-7 window hold the whole disc: 0, 1, 60 and 64 features stay with the lane, 65, 70 and 300 go to the wave
    assert want["n_cand"][:, 7].tolist() == list(DISC_SIZES)
    assert any(n <= 64 for n in DISC_SIZES[2:]) and any(64 < n <= 70 for n in DISC_SIZES) and want["n_cand"].max() > 256
    st = fs.unpack_table(want["table"])["status"]
    assert {4, 5, 6, 7} <= set(st.ravel().tolist())
    same(fs.fuse_sim3_eval(ctx, sc, want_uv=True), want, "disc")


def test_repeated_calls_and_bad_arguments_on_one_context(ctx, mixed):
    sc, _, _, _, want = mixed
    small = sc.subset([1, 2], 300)
    wsmall = fs.fuse_sim3_eval_host(small, want_uv=True)
    for rep in range(3):
        same(fs.fuse_sim3_eval(ctx, sc, want_uv=rep != 1), want, f"repeat {rep}")
        same(fs.fuse_sim3_eval(ctx, small, want_uv=True), wsmall, f"small {rep}")
    from ccm_slam_amd._lib import CcmError
    for name, b in bad_argument_cases() + [("K * P beyond INT32_MAX", huge_product_case())]:
        table = np.zeros(max(min(b.K * b.P, 1 << 20), 1), np.uint32); nv = np.zeros(b.K, np.int32); nh = np.zeros(b.K, np.int32)
        assert fs._dev().ccm_fuse_sim3_eval(ctx.handle, *b.args(), fs._p(table), fs._p(nv), fs._p(nh), None) == -1, name     # CCM_E_ARG
    same(fs.fuse_sim3_eval(ctx, small, want_uv=True), wsmall, "after the refusals")


def test_two_contexts_on_two_threads(mixed):
    from ccm_slam_amd._lib import Context
    sc, _, _, _, want = mixed
    subs = [sc.subset([0, 2, 4], 1500), sc.subset([1, 3, 5, 7], 2500)]
    wants = [fs.fuse_sim3_eval_host(s, want_uv=True) for s in subs]
    errs = []

    def run(j):
        try:
            c = Context(0)
            try:
                for _ in range(4):
                    same(fs.fuse_sim3_eval(c, subs[j], want_uv=True), wants[j], f"thread {j}")
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


def test_mirror_on_the_device_through_eight_fuse_calls(ctx, frames, mixed):
    """the CPU file's walk on a batch evaluated on the device; without the reference's library on this machine, against the mirror on the host evaluator"""
    sc, s, S16, which, want = mixed
    dev = fs.SearchAndFuseBatch(ctx, sc)
    try:
        assert np.array_equal(dev.table()["table"], want["table"])
        if os.path.exists(trm.LIB):
            walk(dev, sc, s, S16, frames, which, C.CDLL(trm.LIB), want["table"])
        else:
            host = fs.SearchAndFuseBatch(None, sc)
            rng = np.random.default_rng(5)
            skip = np.zeros(sc.P, np.uint8); now = s["pdesc"].copy()
            for k in range(sc.K):
                a, b = dev.resolve(k, skip, now), host.resolve(k, skip, now)
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and dev.n_reeval() == host.n_reeval()
                fused = np.flatnonzero(a[1] >= 0)
                now[fused[0::3]] = frames[which[k]][1][a[1][fused[0::3]]]
                skip[fused[1::3]] = 1; skip[rng.choice(sc.P, 15, replace=False)] = 1
            assert host.n_reeval() > 100
            host.close()
    finally:
        dev.close()
