"""GPU box: host-to-host time of the guided search's device call (ccm_frame_guided_search: gates, windows and Hamming distances of all P slots in one call)
against (a) the host evaluator on ONE thread (ccmh_guided_search_host: csrc/guided_search_math.h, a host grid built per call, host popcounts) and (b) what the
tree offered before the call existed: the gates on the host, then ccm_frame_window_search on the searched slots.  For (b) the gates are the same header on one
thread (ccmh_guided_search_host against a frame without features, which evaluates the gates and nothing else) and the compaction of the searched slots is numpy.

Medians of 200 repetitions; the three forms alternate, so that all see the same machine state.  Shapes: P = 1000 slots, N = 1000 and 2000 features, th = 10 and 3.
The three forms must return the same lists and distances before anything is timed.  Prints one JSON line; --out FILE also writes it there
(profiles/guided_search_profile.json is the copy DESIGN.md §28 quotes)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ccm_slam_amd import reloc
from ccm_slam_amd._lib import Context
from ccm_slam_amd.frame import FrameGrid

REPS = 200
P = 1000
SHAPES = ((1000, 10.0), (1000, 3.0), (2000, 10.0), (2000, 3.0))
KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
W, H, K = 640, 480, np.array([500, 500, 320, 240], np.float32)
BOUNDS = np.array([0, 0, W, H], np.float32)


def make_scene(seed, N):
    """P points in front of a camera near the origin, nine in ten inside the image and the pyramid's range; N features: one near the projection of every other
    point, at a level near the predicted one, the rest spread over the image (scripts do not import tests: the generator is restated here)."""
    rng = np.random.default_rng(seed)
    sf = np.float32(1.2) ** np.arange(8, dtype=np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = rng.uniform(-0.1, 0.1, 3)
    z = rng.uniform(2.0, 8.0, P)
    x, y = rng.uniform(-0.7, 0.7, P) * z, rng.uniform(-0.5, 0.5, P) * z
    pos = (np.stack([x, y, z], 1) - T[:3, 3]).astype(np.float32)
    d = np.linalg.norm(np.stack([x, y, z], 1), axis=1)
    lvl = rng.uniform(0.0, 7.5, P)
    dmax = (d * 1.2 ** lvl).astype(np.float32)
    dmin = (dmax / 1.2 ** 7).astype(np.float32)
    desc = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    kps = np.zeros(N, KP_DTYPE)
    fdesc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    kps["x"], kps["y"], kps["octave"] = rng.uniform(0, W, N), rng.uniform(0, H, N), rng.integers(0, 8, N)
    near = np.arange(0, P, 2)[:N // 2]
    kps["x"][:near.size] = 500 * x[near] / z[near] + 320 + rng.uniform(-4, 4, near.size)
    kps["y"][:near.size] = 500 * y[near] / z[near] + 240 + rng.uniform(-4, 4, near.size)
    kps["octave"][:near.size] = np.clip(np.ceil(lvl[near]), 0, 7)
    fdesc[:near.size] = desc[near]
    pose = reloc.guided_pose(T, np.log(np.float32(1.2)), sf)
    return pose, pos, dmin, dmax, desc, kps, fdesc, sf


def run(ctx, N, th):
    pose, pos, dmin, dmax, desc, kps, fdesc, sf = make_scene(100 + N, N)
    grid = FrameGrid(ctx, K, np.zeros(0, np.float32), W, H)
    grid.set_keypoints(kps, fdesc)
    none = (np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8))
    cap = 64 * P

    def fused():
        return reloc.guided_search(grid, pose, pos, dmin, dmax, desc, None, th, cap=cap)

    def host():
        return reloc.guided_search_host(kps, fdesc, BOUNDS, K, pose, pos, dmin, dmax, desc, None, th, cap=cap)

    def parent():
        g = reloc.guided_search_host(none[0], none[1], BOUNDS, K, pose, pos, dmin, dmax, desc, None, th, cap=0)     # the gates alone
        q = np.nonzero(g["status"] == reloc.SEARCHED)[0]
        lv = g["level"][q]
        off, idx, dist = grid.window_search(g["u"][q], g["v"][q], np.float32(th) * sf[lv], lv - 1, lv + 1, desc[q])
        return q, off, idx, dist

    for _ in range(3):
        a, b, c = fused(), host(), parent()
    same = all(np.array_equal(a[k], b[k]) for k in ("status", "level", "off", "idx", "dist"))
    q, off, idx, dist = c
    same = same and np.array_equal(np.diff(a["off"])[q], np.diff(off)) and np.array_equal(a["idx"], idx) and np.array_equal(a["dist"], dist)
    assert same, "the three forms disagree"
    t = {"fused": [], "host": [], "parent": []}
    for _ in range(REPS):
        for name, f in (("fused", fused), ("host", host), ("parent", parent)):
            t0 = time.perf_counter(); f(); t[name].append(time.perf_counter() - t0)
    grid.close()
    m = {k: float(np.median(v)) for k, v in t.items()}
    q10 = {k: float(np.percentile(v, 10)) for k, v in t.items()}
    q90 = {k: float(np.percentile(v, 90)) for k, v in t.items()}
    us = lambda s: round(1e6 * s, 1)
    return dict(P=P, N=N, th=th, searched=int((a["status"] == reloc.SEARCHED).sum()), candidates=int(a["n_cand"]), fused_us=us(m["fused"]), host_1thread_us=us(m["host"]),
                host_gate_then_window_search_us=us(m["parent"]), fused_p10_p90_us=[us(q10["fused"]), us(q90["fused"])],
                parent_p10_p90_us=[us(q10["parent"]), us(q90["parent"])], host_over_fused=round(m["host"] / m["fused"], 2),
                parent_over_fused=round(m["parent"] / m["fused"], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = Context(0)
    res = dict(what="ccm_frame_guided_search against ccmh_guided_search_host (one thread) and against host gates + ccm_frame_window_search, through the Python wrappers, "
                    "host to host, medians of %d interleaved repetitions" % REPS, runs=[run(ctx, N, th) for N, th in SHAPES])
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
