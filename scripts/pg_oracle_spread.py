#!/usr/bin/env python3
"""Prints what two builds of the oracle's own source (oracle/Makefile: liboracle.so, -O2 without FMA contraction; liboracle_fast.so, -O3
-march=native) differ by in the pose-graph system (H, b, J of ora_pose_graph_system) on the graphs of tests/test_posegraph_pcg_gpu.py.
ORACLE_BAR_H / _B / _J there are 10 x the largest values; run this again when synth.make_pose_graph or the graph list changes.  CPU only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402
from tests import test_posegraph_pcg_gpu as T  # noqa: E402

worst = np.zeros(3)
for name in T.FAMILIES + ["chain1", "chain2", "chain300"]:
    pg = T._graph(name)
    H1, b1, J1 = oracle.pose_graph_system(pg)
    H2, b2, J2 = oracle.pose_graph_system_fast(pg)
    d = np.array([np.abs(H1 - H2).max() / np.abs(H1).max(), np.abs(b1 - b2).max() / np.abs(b1).max(), np.abs(J1 - J2).max()])
    worst = np.maximum(worst, d)
    print(f"{name:14s} H {d[0]:.3e} of max|H|   b {d[1]:.3e} of max|b|   J {d[2]:.3e}")
print(f"largest        H {worst[0]:.3e}              b {worst[1]:.3e}              J {worst[2]:.3e}")
