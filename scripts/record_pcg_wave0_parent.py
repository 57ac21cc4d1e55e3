"""Writes tests/golden/pcg_wave0_parent.npz, the fixture of tests/test_pcg_wave0_path_gpu.py: what the persistent PCG of the library IN PLACE
computes.  Run it on the MI355X with ccm_slam_amd/libccm_hip.so built from the commit BEFORE the change under test (the parent), never with the
change itself.  usage: python scripts/record_pcg_wave0_parent.py [OUT.npz]

Recorded: the four solves of the 70-camera map (x, iteration counts, lambdas); the first run of LM_CANDIDATES in which a coarse-level trial loads the
saved cluster inverse W (counted from the library's CCM_DBG=trial lines), and run(10) of gba_c3: (LM iterations, trials, CG iterations) and the
sha256 of cameras and points."""
import os
import sys
import tempfile

os.environ["CCM_DBG"] = "trial"   # read once by the library: one stderr line per persistent solve ("... W loaded" / "W factored")
os.environ.pop("CCM_BA_PERS_PREFETCH", None)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from ccm_slam_amd._lib import Context  # noqa: E402
from tests import test_pcg_wave0_path_gpu as T  # noqa: E402


def _with_stderr_captured(fn):
    """fn() with the process's stderr (the native library writes to it) going to a file; returns (fn's result, the text)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            res = fn()
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        return res, tmp.read().decode(errors="replace")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    ctx = Context(0)
    rec = {}
    got, lams, counts, sizes = T.solves(ctx, T.problem("map70"), None)
    print("map70:", counts, "grid", sizes["pers_grid"])
    rec["map70_lam"] = np.array([lams[s] for s in T.SCALES])
    rec["map70_coarse"] = np.array([c for c, _ in T.CASES])
    rec["map70_scale"] = np.array([s for _, s in T.CASES])
    rec["map70_iters"] = np.array([int(got[case][1][1]) for case in T.CASES], np.int32)
    rec["map70_x"] = np.stack([got[case][0] for case in T.CASES])
    for case in T.CASES:
        fl = got[case][1]
        assert fl[2] == 0 and fl[3] == 0 and fl[1] > 0, (case, fl)
    for name, iters in T.LM_CANDIDATES:
        (cnt, cam_sha, pts_sha, n_pers, n_spmv), log = _with_stderr_captured(lambda: T.lm_run(ctx, T.problem(name), iters))
        loads = sum(1 for ln in log.splitlines() if "trial:" in ln and "W loaded" in ln and "coarse off" not in ln)
        print(f"{name}: run({iters}) counts {cnt}, persistent launches {n_pers}, multi-kernel {n_spmv}, coarse-level trials that loaded W: {loads}")
        print("".join("    " + ln + "\n" for ln in log.splitlines() if "trial:" in ln), end="")
        if loads > 0 and n_spmv == 0:
            rec.update(lm_case=np.array(name), lm_iters=np.array(iters), lm_w_loads=np.array(loads), lm_counts=np.array(cnt, np.int32), lm_cam_sha256=np.array(cam_sha), lm_pts_sha256=np.array(pts_sha))
            break
    else:
        raise SystemExit("no candidate run has a coarse-level trial that loads W")
    (cnt, cam_sha, pts_sha, n_pers, n_spmv), _ = _with_stderr_captured(lambda: T.lm_run(ctx, T.problem("gba_c3"), 10))
    print(f"gba_c3: run(10) counts {cnt}, persistent launches {n_pers}, multi-kernel {n_spmv}")
    assert n_pers > 0 and n_spmv == 0
    rec.update(c3_counts=np.array(cnt, np.int32), c3_cam_sha256=np.array(cam_sha), c3_pts_sha256=np.array(pts_sha))
    ctx.close()
    np.savez(out_path, **rec)
    print("wrote", out_path, os.path.getsize(out_path), "bytes")


if __name__ == "__main__":
    main()
