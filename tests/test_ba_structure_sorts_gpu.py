"""The sorts and the pair emit of the BA structure build (ccm_slam_amd/csrc/ba_sort.h, ba_build.hip, ba_structure.hip).

The build's stable radix sorts run one of rocPRIM's three paths (one workgroup up to 1024 items, merge passes, onesweep); which one is a matter of
size and of CCM_BA_SORT, read at every ccm_ba_create: unset = onesweep from a measured size on, "merge" = rocPRIM's own choice, "onesweep" = no merge
path at any size.  All three are stable, so no array of the handle may depend on the setting: compared here as bytes, at the sizes where the path changes
against the numpy restatement of test_ba_structure_gpu.py, and end to end through a short LM run.  The pair emit (a workgroup per 32 landmarks, rows through
LDS in tiles of 256, a pair finds its row by binary search) is checked at its edges against the same restatement."""
import numpy as np
import pytest

from ccm_slam_amd import optimizer, synth
from test_ba_structure_gpu import check, dev_array

pytestmark = pytest.mark.gpu

SETTINGS = [None, "merge", "onesweep"]
# every array ccm_ba_debug_array knows (the name list of test_ba_structure_gpu.check); one a handle does not carry reads as empty
ARRAYS = ["sizes", "slot_cam", "slot_pt", "loc_edge_orig", "pt_off", "ed_cam", "ed_cslot", "ed_pt", "cam_off", "cam_edge", "cam_pt", "rowblk_off", "row_off",
          "row_col", "inst_off", "inst_a", "inst_c", "inst_al", "blk_i", "blk_j", "chunk_off", "row_blk", "obs", "info", "cam_oi", "pers_coff", "pers_cij",
          "pers_cblk", "pers_uoff", "pers_ucol", "pers_loc", "unit_tab", "row_unit_off", "blk_unit0", "cb_off", "cb_ab", "cb_ent"]


def use_sort(monkeypatch, setting):
    if setting is None:
        monkeypatch.delenv("CCM_BA_SORT", raising=False)
    else:
        monkeypatch.setenv("CCM_BA_SORT", setting)


def structure_bytes(ctx, prob):
    h = optimizer.BAHandle(ctx, prob)
    out = {nm: dev_array(h, nm, np.uint8) for nm in ARRAYS}
    h.close()
    return out


def with_edges(prob, keep):
    """the problem with the edges `keep` (indices, in this order) only"""
    out = dict(prob, n_edge=int(len(keep)))
    for nm in ("e_cam", "e_pt", "e_obs", "e_info"):
        out[nm] = np.ascontiguousarray(prob[nm][keep])
    if prob.get("e_level") is not None:
        out["e_level"] = np.ascontiguousarray(np.asarray(prob["e_level"])[keep])
    return out


def lba_c2_second_stage():
    prob = synth.make_ba_config("lba_c2")
    lvl = np.zeros(prob["n_edge"], np.uint8)
    lvl[np.random.default_rng(5).random(prob["n_edge"]) < 0.07] = 1   # outliers moved to level 1, as in test_ba_structure_gpu.py
    return dict(prob, e_level=lvl)


@pytest.mark.parametrize("which", ["multi_agent", "lba_c2"])
def test_every_array_is_the_same_bytes_under_every_sort_setting(ctx, which, monkeypatch):
    prob = synth.make_ba_problem(n_agents=3, kfs_per_agent=60, n_points=6000, seed=21, n_fixed=1) if which == "multi_agent" else lba_c2_second_stage()
    got = {}
    for s in SETTINGS:
        use_sort(monkeypatch, s)
        got[s] = structure_bytes(ctx, prob)
    assert got[None]["inst_a"].size and got[None]["row_col"].size
    for s in SETTINGS[1:]:
        for nm in ARRAYS:
            assert np.array_equal(got[None][nm], got[s][nm]), (s, nm)


def _a_handful_over_one_workgroup():
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=17, n_points=900, seed=3)
    assert prob["n_edge"] > 1029
    return with_edges(prob, np.arange(1029))      # rocPRIM sorts up to 1024 items in one workgroup


SIZE_CASES = {
    "no_edge": lambda: synth.make_ba_problem(n_agents=1, kfs_per_agent=2, n_points=60, seed=1),      # (two keyframes share no landmark: nothing to sort)
    "one_workgroup": lambda: synth.make_ba_problem(n_agents=1, kfs_per_agent=6, n_points=150, seed=4),
    "a_few_thousand": lambda: synth.make_ba_problem(n_agents=1, kfs_per_agent=17, n_points=900, seed=3),
    "a_handful_over_one_workgroup": _a_handful_over_one_workgroup,
}


@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("case", list(SIZE_CASES))
def test_structure_at_the_sizes_where_the_sort_path_changes(ctx, case, setting, monkeypatch):
    prob = SIZE_CASES[case]()
    if case == "no_edge": assert prob["n_edge"] == 0
    if case == "one_workgroup": assert 0 < prob["n_edge"] < 1024
    if case == "a_few_thousand": assert 2000 < prob["n_edge"] < 20000
    use_sort(monkeypatch, setting)
    check(ctx, prob)


def _several_fixed_cameras():
    return synth.make_ba_problem(n_agents=1, kfs_per_agent=24, n_points=700, seed=5, n_fixed=8, fixed_mode="tail")


def _one_camera_twice():
    # a landmark observed twice by the same camera: the row of the first of the two skips the second (ic == ia), and the rows before pair with both
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=12, n_points=300, seed=6, n_fixed=1)
    track = np.bincount(prob["e_pt"], minlength=prob["n_pt"])
    free = np.asarray(prob["cam_fixed"])[prob["e_cam"]] == 0
    long_enough = np.flatnonzero(free & (track[prob["e_pt"]] >= 4))
    cam_rank = np.array([np.sum(prob["e_cam"][prob["e_pt"] == prob["e_pt"][e]] < prob["e_cam"][e]) for e in long_enough])
    first, middle, last = long_enough[cam_rank == 0][0], long_enough[cam_rank == 1][1], long_enough[cam_rank >= 3][2]   # copies at the head, inside and at the tail of a row list
    fixed_edge = np.flatnonzero(~free)[0]                                                                               # and an observation of a fixed camera twice
    return with_edges(prob, np.concatenate([np.arange(prob["n_edge"]), [first, middle, middle, last, fixed_edge]]))


def _one_observation_and_none():
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=12, n_points=300, seed=7, n_fixed=1)
    lvl = np.zeros(prob["n_edge"], np.uint8)
    of = lambda p: np.flatnonzero(prob["e_pt"] == p)
    lvl[of(11)[1:]] = 1          # a landmark with one observation left: no pair
    lvl[of(12)[:-1]] = 1         # (its last one)
    lvl[of(40)] = 1              # a landmark that loses all its edges to level 1
    lvl[of(299)] = 1             # (the last landmark)
    return dict(prob, e_level=lvl)


def _longer_than_a_tile():
    # landmarks with more observations than the emit's tile of 256 rows: their rows span tiles.  The generator keeps what a camera sees (a few dozen keyframes
    # per track), so two landmarks are given an observation in every keyframe by hand (the structure does not look at the measurements)
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=300, n_points=150, seed=3, n_fixed=2)
    add_cam, add_pt = [], []
    for p in (5, 149):
        missing = np.setdiff1d(np.arange(prob["n_cam"]), prob["e_cam"][prob["e_pt"] == p])
        add_cam.append(missing); add_pt.append(np.full(missing.size, p))
    add_cam, add_pt = np.concatenate(add_cam).astype(prob["e_cam"].dtype), np.concatenate(add_pt).astype(prob["e_pt"].dtype)
    out = dict(prob, n_edge=int(prob["n_edge"] + add_cam.size))
    out["e_cam"] = np.concatenate([prob["e_cam"], add_cam]); out["e_pt"] = np.concatenate([prob["e_pt"], add_pt])
    out["e_obs"] = np.concatenate([prob["e_obs"], np.column_stack([100.0 + add_cam, 200.0 + add_pt])])
    out["e_info"] = np.concatenate([prob["e_info"], np.ones(add_cam.size)])
    if prob.get("e_level") is not None:
        out["e_level"] = np.concatenate([np.asarray(prob["e_level"], np.uint8), np.zeros(add_cam.size, np.uint8)])
    assert np.bincount(out["e_pt"]).max() == 300
    return out


EMIT_CASES = {
    "several_fixed_cameras": _several_fixed_cameras,
    "one_camera_twice": _one_camera_twice,
    "one_observation_and_none": _one_observation_and_none,
    "longer_than_a_tile": _longer_than_a_tile,
}


@pytest.mark.parametrize("case", list(EMIT_CASES))
def test_pair_emit_at_its_edges(ctx, case):
    check(ctx, EMIT_CASES[case]())


@pytest.mark.parametrize("rank", [0, 1])
def test_pair_emit_of_a_two_rank_shard(ctx, rank):
    prob = synth.make_ba_problem(n_agents=2, kfs_per_agent=40, n_points=3000, seed=8, n_fixed=1)
    check(ctx, prob, rank, 2)    # own pairs with values, and the keys of all landmarks without


def test_a_short_lm_run_is_the_same_under_every_sort_setting(ctx, monkeypatch):
    """The structure feeds every summation order, so equal structures mean equal bits.  gba_c3 has more observations than the size from which the build takes
    onesweep (and fewer than rocPRIM's own limit), so unset and "merge" sort its observations by different paths."""
    prob = synth.make_ba_config("gba_c3")
    assert (1 << 18) < prob["n_edge"] < (1 << 20)
    got = {}
    for s in SETTINGS:
        use_sort(monkeypatch, s)
        h = optimizer.BAHandle(ctx, prob)
        structure = {nm: dev_array(h, nm, np.uint8) for nm in ("loc_edge_orig", "cam_edge", "inst_off", "inst_a", "inst_c", "row_col", "row_blk", "unit_tab")}
        st = h.run(3)
        cam, pts, _, _ = h.download()
        got[s] = ((st.iters_done, st.lm_trials, st.pcg_iters), cam, pts, structure)
        h.close()
    assert got[None][0][0] > 0 and got[None][0][2] > 0
    for s in SETTINGS[1:]:
        assert got[s][0] == got[None][0], s
        assert got[s][1].tobytes() == got[None][1].tobytes() and got[s][2].tobytes() == got[None][2].tobytes(), s
        for nm, a in got[None][3].items():
            assert np.array_equal(a, got[s][3][nm]), (s, nm)
