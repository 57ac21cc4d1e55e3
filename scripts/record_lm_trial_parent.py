"""Writes tests/golden/lm_trial_parent.npz, the fixture of tests/test_lm_trial_parent_gpu.py: what the LM runs of its CASES hand their caller with the
library IN PLACE, and the launches they count in every CCM_K_BA_* class.  Run it on the MI355X with ccm_slam_amd/libccm_hip.so built from the commit BEFORE
the change under test (the parent), never with the change itself.  usage: python scripts/record_lm_trial_parent.py [OUT.npz]

Every case runs twice.  Counts, history() and launches must agree between the two runs (the script stops otherwise).  A case whose downloaded cameras or
digests differ between them is a finding about the parent: it is reported, marked <case>_reproducible = False and recorded without those keys."""
import os
import sys

for _k in ("CCM_BA_CHOLREG", "CCM_BA_NO_PERSIST", "CCM_BA_COARSE", "CCM_BA_PERS_CAMUPD", "CCM_BA_PERS_PREFETCH", "CCM_BA_COARSE_AGG", "CCM_BA_TEST_ABORT", "CCM_BA_SORT"):
    os.environ.pop(_k, None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ccm_slam_amd._lib import Context  # noqa: E402
from tests import test_lm_trial_parent_gpu as T  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    ctx = Context(0)
    rec = {"ba_classes": np.array(T.BA_CLASSES)}
    for name in T.CASES:
        one, two = T.lm_run(ctx, name), T.lm_run(ctx, name)
        sz = one["sizes"]
        print(f"{name}: Cp {sz['Cp']}, grid {sz['pers_grid']}, counts {one['counts'].tolist()}, trials per iteration {one['hist_trials'].tolist()}, "
              f"launches {dict(zip(T.BA_CLASSES, one['launches'].tolist()))}")
        for key in T.ALWAYS_KEYS:
            assert T.same(one[key], two[key]), (name, key, one[key], two[key])
        differ = [key for key in T.BYTE_KEYS if not T.same(one[key], two[key])]
        if differ:
            print(f"{name}: NOT reproducible on this library: {differ} differ between two runs; recorded by counts, history and launches only")
        rec[name + "_reproducible"] = np.array(not differ)
        for key in T.ALWAYS_KEYS + (() if differ else T.BYTE_KEYS):
            rec[name + "_" + key] = one[key]
        if T.CASES[name][0] == ("map70",):
            assert one["counts"][1] > one["counts"][0], (name, "no rejected trial: raise ITERS_MAP70", one["counts"])
    ctx.close()
    np.savez(out_path, **rec)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
