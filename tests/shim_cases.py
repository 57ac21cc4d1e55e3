"""Small maps with bad keyframes and bad points for the class-API comparisons of shim/Optimizer_hip.cpp (tests/test_shim_gpu.py), shared with
scripts/shim_state_record.py, which records what a given build of the shim leaves on the same maps (tests/golden/shim_optimizer_parent.npz).

cases() maps a name to (flat map, call): `call(graph)` runs one Optimizer entry point on a fresh oracle.mapgraph.MapGraph of that map."""
import functools

import numpy as np

from ccm_slam_amd import synth
from oracle import mapgraph as mg


def sim3_of_pose(T, s=1.0):
    from oracle import to_se3quat
    q = to_se3quat(T)[0]
    return np.concatenate([q, [s]])


def global_ba_map():
    """two agents, 24 keyframes, 600 points; keyframes 5 and 17 and every seventh point are bad.  Keyframe 12 is agent 1's first: its fixed camera."""
    prob = synth.make_ba_problem(n_agents=2, kfs_per_agent=12, n_points=600, seed=4, n_fixed=1)
    flat = mg.flat_from_ba_problem(prob, n_agents=2)
    flat["kf_bad"][[5, 17]] = 1
    flat["mp_bad"][::7] = 1
    return flat


def local_ba_map():
    """one agent, 14 keyframes, 500 points, covisibility threshold 5; keyframe 4 and every ninth point are bad.  Keyframe 4 is inside the window of keyframe 2."""
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=14, n_points=500, seed=12, n_fixed=1, mean_track=6)
    flat = mg.flat_from_ba_problem(prob)
    flat["cov_th"] = 5
    flat["kf_bad"][4] = 1
    flat["mp_bad"][::9] = 1
    return flat


def essential_graph_map():
    """one agent driving a closed loop of 24 keyframes, 1200 points, every eleventh point bad; every keyframe good"""
    prob = synth.make_ba_problem(n_agents=1, kfs_per_agent=24, n_points=1200, seed=33, n_fixed=1)
    flat = mg.flat_from_ba_problem(prob)
    flat["mp_bad"][::11] = 1
    return flat


def essential_graph_call(flat, map_fusion):
    T = flat["kf_Tcw"]
    shift = lambda k: np.r_[np.zeros(4), [0.01 * (k - 18), -0.004 * (k - 18), 0.002], [0.01]]   # the loop closure's correction: a drift in t, 1 % in scale
    corrected = [(k, sim3_of_pose(T[k]) + shift(k)) for k in range(19, 24)]
    noncorrected = [(k, sim3_of_pose(T[k])) for k in range(19, 24)]
    connections = [(23, 0), (23, 1), (22, 0), (21, 2)]
    loop_edges = [(12, 4)]
    return lambda g: g.essential_graph(0, 23, () if map_fusion else corrected, () if map_fusion else noncorrected, connections, loop_edges,
                                       fix_scale=False, map_fusion=map_fusion)


CASE_NAMES = ("gba_fusion", "gba_fusion_plain", "gba_fusion_parked", "gba_client", "gba_client_parked", "lba_7", "lba_2", "ess_loop", "ess_fusion")


@functools.lru_cache(maxsize=None)
def cases():
    a, b, c = global_ba_map(), local_ba_map(), essential_graph_map()
    return {
        "gba_fusion": (a, lambda g: g.map_fusion_gba(0, 4)),
        "gba_fusion_plain": (a, lambda g: g.map_fusion_gba(0, 4, robust=False)),
        "gba_fusion_parked": (a, lambda g: g.map_fusion_gba(0, 3, loop_kf=(3, 0))),
        "gba_client": (a, lambda g: g.bundle_adjustment_client(0, 4)),
        "gba_client_parked": (a, lambda g: g.bundle_adjustment_client(1, 4)),     # nLoopKF = (0, 0) is not client 1's origin (0, 1): results go to mTcwGBA / mPosGBA
        "lba_7": (b, lambda g: g.local_ba(7, client_id=0)),
        "lba_2": (b, lambda g: g.local_ba(2, client_id=0)),
        "ess_loop": (c, essential_graph_call(c, False)),
        "ess_fusion": (c, essential_graph_call(c, True)),
    }


def run(lib_path, name):
    """what `lib_path` leaves in the map of case `name`: the arrays of MapGraph.state()"""
    flat, call = cases()[name]
    g = mg.MapGraph(lib_path, flat)
    try:
        assert call(g) == 0, name
        return g.state()
    finally:
        g.close()
