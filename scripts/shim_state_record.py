"""GPU box: record what this checkout's shim/Optimizer_hip.cpp (shim/liboptimizer_hip_shim.so) leaves in the map on every case of tests/shim_cases.py.

    shim_state_record.py [out.npz]           record (default tests/golden/shim_optimizer_parent.npz); keys are "<case>/<state array>"
    shim_state_record.py --check file.npz    record again and list the arrays that differ from file.npz (exit 1 if any does)

The committed fixture was recorded with this script from a checkout of the commit BEFORE the graph walks of the shim were rewritten, with tests/shim_cases.py
copied into it: tests/test_shim_gpu.py asserts that the rewritten walks leave the same bits (same vertices, same edges, same order)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from oracle import mapgraph as mg
from tests import shim_cases as sc


def record():
    out = {}
    for name in sc.CASE_NAMES:
        for k, v in sc.run(mg.SHIM_LIB, name).items():
            out[f"{name}/{k}"] = v
    return out


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--check":
        old, new = np.load(sys.argv[2]), record()
        diff = [k for k in new if not np.array_equal(old[k], new[k])]
        for k in diff:
            print(f"differs: {k}  max |d| = {np.abs(old[k].astype(np.float64) - new[k].astype(np.float64)).max():.3e}")
        print(f"{len(new) - len(diff)} of {len(new)} arrays repeat bit for bit")
        sys.exit(1 if diff else 0)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "shim_optimizer_parent.npz")
    np.savez_compressed(path, **record())
    print(f"{path}: {os.path.getsize(path)} bytes")
