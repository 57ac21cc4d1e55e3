"""GPU: the six projected searches (ccm_fuse_sim3_eval, ccm_fuse_pose_eval, their resident forms, ccm_sim3_project_eval_resident, ccm_sim3_pair_eval_resident) are
one staged block (FuseBlock, csrc/stage_blocks.h) in six forms.  Here they alternate through ONE context's scratch and ONE store, at sizes that grow
and then shrink (K 1 / 3 / 3 keyframes, P 1 / 257 / 600 points: a single pair, a full tile and a tail of one, a partly dead last wave), so that every form finds the
buffers as another form of another size left them: segments it does not have next to segments it has, a call without uv right behind one with it.  One keyframe has
no features, the masks' lengths are no multiple of four, one pair job list has an empty job.  Every table, counter and uv equals the host evaluator's (exact)."""
import numpy as np
import pytest

from kfstore_cases import same_result
from sim3_search_cases import IDENT12

N_FEAT = 301
SIZES = dict(tiny=([0], 1), mid=([0, 1, 2], 257), big=([0, 1, 2], 600))
POSE_JOBS = dict(tiny=[(0, 0, 1)], mid=[(0, 0, 257), (1, 0, 100), (2, 100, 157)], big=None)          # None: the scene's own, 2 x 257 + 343
PAIR_JOBS = dict(tiny=[(0, 0, 1)], mid=[(2, 0, 257), (0, 0, 0), (0, 57, 200)], big=[(0, 0, 600), (2, 300, 300)])


def _without_features(sc, k):
    """the fuse_sim3.Scene `sc` with keyframe k's features taken out"""
    from ccm_slam_amd import fuse_sim3 as fs
    a, b, end = int(sc.feat_off[k]), int(sc.feat_off[k + 1]), int(sc.feat_off[sc.K])
    keep = np.r_[0:a, b:end]
    off = sc.feat_off.copy(); off[k + 1:] -= b - a
    co = sc.cell_off.reshape(sc.K, -1).copy(); co[k] = 0
    return fs.Scene(sc.rec, off, sc.feat_xy.reshape(-1, 2)[keep], sc.feat_octave[keep], sc.feat_desc.reshape(-1, 32)[keep], co, sc.cell_idx[keep], sc.Scw, sc.scale_factors,
                    sc.log_sf, sc.th, sc.pos, sc.normal, sc.min_dist, sc.max_dist, sc.pt_desc)


def _pair_scene(sim, jobs):
    """SearchBySim3 jobs on the keyframes and points of `sim`: the source pose is the keyframe's Scw, the transform the identity"""
    from ccm_slam_amd import sim3_search as ss
    S = sim.Scw.reshape(-1, 3, 4)
    full = [(k, sim.rec.reshape(-1, 10)[k, :4], np.concatenate([S[k, :, :3].reshape(-1), S[k, :, 3]]), IDENT12, pt0, n) for k, pt0, n in jobs]
    return ss.PairScene(sim, 7.5, sim.pos, sim.min_dist, sim.max_dist, sim.pt_desc, full)


@pytest.mark.gpu
def test_the_six_calls_alternate_through_one_scratch_at_growing_and_shrinking_sizes():
    from ccm_slam_amd import fuse_pose as fp, fuse_sim3 as fs, kfstore as ks, sim3_search as ss
    from ccm_slam_amd._lib import Context
    sim_full = _without_features(fs.make_scene(3, 600, n_feat=N_FEAT, seed=71), 1)
    pose_full = fp.make_scene(2, 257, 343, n_feat=N_FEAT, seed=72)
    rng = np.random.default_rng(73)
    cases = {}
    for tag, (kfs, P) in SIZES.items():
        sim = sim_full.subset(kfs, P)
        pose = pose_full.subset(kfs, P, jobs=POSE_JOBS[tag])
        masks = [(rng.random(n) < 0.3).astype(np.uint8) for n in np.diff(sim.feat_off)]
        assert sum(m.size for m in masks) % 4 != 0
        pair = _pair_scene(sim, PAIR_JOBS[tag])
        cases[tag] = dict(sim=sim, pose=pose, masks=masks, pair=pair, want=dict(
            sim3=fs.fuse_sim3_eval_host(sim, want_uv=True), pose=fp.fuse_pose_eval_host(pose, want_uv=True),
            project=ss.project_eval_host(sim, masks, want_uv=True), pair=ss.pair_eval_host(pair, want_uv=True)))
    big = cases["big"]["want"]
    assert all(big[f]["n_hit"].sum() > 20 for f in ("sim3", "pose", "project", "pair")) and big["sim3"]["n_hit"][1] == 0
    assert not np.array_equal(big["sim3"]["table"], big["project"]["table"])      # the masks take candidates away

    ctx = Context(0)
    store = ks.KeyFrameStore(ctx, 8, N_FEAT)
    try:
        store.add_scene([10, 11, 12], sim_full)
        store.add_scene([20, 21, 22], pose_full)
        n = 0
        for rnd, tag in enumerate(("tiny", "mid", "big", "mid", "tiny")):
            c = cases[tag]
            sk = [10 + k for k in SIZES[tag][0]]; pk = [20 + k for k in SIZES[tag][0]]
            calls = [("sim3", lambda uv: fs.fuse_sim3_eval(ctx, c["sim"], want_uv=uv)),
                     ("pose", lambda uv: ks.fuse_pose_eval_resident(ctx, store, pk, c["pose"], want_uv=uv)),
                     ("project", lambda uv: ss.project_eval_resident(ctx, store, sk, c["sim"], c["masks"], want_uv=uv)),
                     ("pose", lambda uv: fp.fuse_pose_eval(ctx, c["pose"], want_uv=uv)),
                     ("pair", lambda uv: ss.pair_eval_resident(ctx, store, sk, c["pair"], want_uv=uv)),
                     ("sim3", lambda uv: ks.fuse_sim3_eval_resident(ctx, store, sk, c["sim"], want_uv=uv)),
                     ("project", lambda uv: ss.project_eval_resident(ctx, store, sk, c["sim"], c["masks"], want_uv=uv))]
            for i in range(len(calls)):                                            # seven calls a round: every call's uv flips from one round to the next
                form, call = calls[(i + rnd) % len(calls)]
                uv = n % 2 == 1
                got = call(uv)
                assert ("uv" in got) == uv
                same_result(got, c["want"][form], (rnd, tag, form, "uv" if uv else "no uv"))
                n += 1
    finally:
        store.close()
        ctx.close()
