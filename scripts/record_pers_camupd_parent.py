"""Writes tests/golden/pers_camupd_parent.npz, the fixture of tests/test_pers_camupd_gpu.py: what run(8) of map70 and of map179 hand their caller with the
library IN PLACE.  Run it on the MI355X with ccm_slam_amd/libccm_hip.so built from the commit BEFORE the change under test (the parent), never with the change
itself.  usage: python scripts/record_pers_camupd_parent.py [OUT.npz]

Recorded per map: (LM iterations, trials, CG iterations), history() (chi2, lambda and trials per LM iteration), the downloaded cameras, and the sha256 of the
downloaded points, chi2 per edge and depth flags."""
import os
import sys

os.environ.pop("CCM_BA_PERS_CAMUPD", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ccm_slam_amd._lib import Context  # noqa: E402
from tests import test_pers_camupd_gpu as T  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    ctx = Context(0)
    rec = {}
    for name in T.MAPS:
        res = T.lm_run(ctx, name, None, read_flags=False)   # (the flags' test hook may be younger than the library in place)
        again = T.lm_run(ctx, name, None, read_flags=False)
        print(f"{name}: {res['free_cams']} free cameras, grid {res['pers_grid']}, counts {res['counts'].tolist()}, trials per iteration {res['hist_trials'].tolist()}, "
              f"launches {res['launches']}")
        assert res["launches"]["BA_PCG_PERSIST"] == int(res["counts"][1]) and res["launches"]["BA_PCG_SPMV"] == 0, res["launches"]
        one, two = T.fixture_record(res), T.fixture_record(again)
        for key, val in one.items():
            assert val.tobytes() == two[key].tobytes(), (name, key)   # the recording is reproducible on this library
            rec[name + "_" + key] = val
    ctx.close()
    np.savez(out_path, **rec)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
