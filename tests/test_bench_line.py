"""bench.py's output contract (CPU): the last stdout line is ONE compact JSON line below 4 KB — round 5's 21 KB line was lost by the driver's parser —
and the long record goes to a side file.  The compacting function is fed the committed long records of earlier rounds."""
import glob
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LONG_RECORDS = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[45]*_bench_line.json")))


@pytest.mark.parametrize("path", LONG_RECORDS[-6:], ids=lambda p: os.path.basename(p))
def test_compact_line_is_small_and_complete(path):
    import bench
    full = json.load(open(path))
    line = bench.compact_line(full, os.path.join(ROOT, "bench_extra.json"))
    assert "\n" not in line and len(line) < 4000
    c = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "extra_file"):
        assert k in c, k
    assert c["value"] == full["value"] and c["ms_per_step"] == full["ms_per_step"]
    assert c["config"]["workload"].startswith("gba_c")
    if full.get("roofline"):
        r = c["roofline"]
        assert r["bound"] in ("hbm", "mfma") and r["unit"] == "GB/s"
        assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
    if full.get("cpu_baseline"):
        assert {"value", "unit", "cores", "kind", "sample"} <= set(c["cpu_baseline"])


def test_an_oversized_record_still_yields_a_small_line():
    import bench
    full = json.load(open(LONG_RECORDS[-1]))
    full["config"]["workload"] = "x" * 5000
    full["roofline"]["bound"] = "y" * 5000
    line = bench.compact_line(full, "bench_extra.json")
    json.loads(line)
    assert len(line) < 4000 + 5000   # the workload string is the caller's; everything optional is gone
    assert "roofline_trial" not in json.loads(line)


def test_stdout_is_one_json_line_and_stderr_is_empty():
    """the part of the contract that runs without a GPU: --plumbing-only goes through the same descriptor handling as the full run"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--plumbing-only"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stderr == ""
    lines = out.stdout.splitlines()
    assert len(lines) == 1
    assert json.loads(lines[-1])["plumbing"] == "ok"


def test_steps_below_one_are_refused():
    """--steps is the number of timed steps and ms_per_step is taken over them: zero steps cannot yield a figure"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 2 and "--steps" in out.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """A plain run: the headline line of the K timed steps and nothing of --full; --dump-outputs leaves what the last step returns to its caller,
    float32 / float64 only, shaped like the problem the seeded workload describes."""
    import numpy as np
    from ccm_slam_amd import synth
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "lba_c2", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 1
    c = json.loads(lines[0])
    assert (c["steps"], c["warmup"]) == (3, 1) and c["ms_per_step"] > 0 and c["value"] > 0
    assert (c["unit"], c["higher_is_better"], c["dtype"]) == ("LM iter/s", True, "f64")
    assert not {"roofline", "roofline_trial", "cpu_baseline"} & set(c)
    got = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert set(got) == {"cam_qt", "pt_xyz", "chi2_per_edge", "depth_positive", "stats", "chi2_per_iteration"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    prob = synth.make_ba_config("lba_c2")
    assert got["cam_qt"].shape == (prob["n_cam"], 7) and got["pt_xyz"].shape == (prob["n_pt"], 3)
    assert got["chi2_per_edge"].shape == got["depth_positive"].shape == (prob["n_edge"],)
    assert int(got["stats"][0]) == got["chi2_per_iteration"].size == c["config"]["lm_iterations_per_step"]
    assert np.all(np.isfinite(got["cam_qt"])) and np.all(np.isfinite(got["chi2_per_edge"]))


def test_side_files_fall_back_to_the_temporary_directory(tmp_path, monkeypatch):
    """bench.py may be run by a user who cannot write the checkout: its log and long record then go to new files in the temporary directory, and the
    result line names them by absolute path."""
    import tempfile
    import bench
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    fd, path = bench.open_side_file("bench_log.txt")
    os.close(fd)
    assert path == str(tmp_path / "bench_log.txt") and bench.shown_path(path) == "bench_log.txt"
    not_a_dir = tmp_path / "file"
    not_a_dir.write_text("")
    monkeypatch.setattr(bench, "ROOT", str(not_a_dir))          # nothing can be created below it, whoever runs the test
    fd, path = bench.open_side_file("bench_log.txt")
    try:
        os.write(fd, b"x")
        assert os.path.dirname(path) == tempfile.gettempdir() and os.path.basename(path).startswith("bench_log_") and path.endswith(".txt")
        assert bench.shown_path(path) == path
    finally:
        os.close(fd)
        os.remove(path)


def test_dump_outputs_needs_a_single_rank(tmp_path):
    """ccm_ba_download is collective across the ranks of a sharded handle: a dump from an N-rank run is refused before any device work"""
    dump = tmp_path / "dump"
    for extra, env in ((["--gpus", "2"], {}), ([], {"WORLD_SIZE": "2"})):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra, "--dump-outputs", str(dump)], capture_output=True, text=True,
                             timeout=120, cwd=ROOT, env=dict(os.environ, **env))
        assert out.returncode == 2 and "--dump-outputs needs a single rank" in out.stderr, out.stderr[-2000:]
    assert not dump.exists()


def test_dump_cap_keeps_a_fixed_sample_within_the_cap(tmp_path):
    """Above the cap every per-landmark and per-observation array keeps the same seeded rows, their indices beside them, and the .npy files together
    stay within the cap; below it the arrays pass unchanged."""
    import numpy as np
    import bench
    rng = np.random.default_rng(0)
    n_cam, n_pt, n_edge = 2000, 200_000, 1_200_000
    arrays = {"cam_qt": rng.random((n_cam, 7)), "pt_xyz": rng.random((n_pt, 3)), "chi2_per_edge": rng.random(n_edge),
              "depth_positive": (rng.random(n_edge) > 0.1).astype(np.float32), "stats": rng.random(7), "chi2_per_iteration": rng.random(12)}
    cap = 4 << 20
    out = bench.cap_outputs(arrays, cap)
    for name, a in out.items():
        np.save(tmp_path / (name + ".npy"), np.ascontiguousarray(a))
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= cap
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    pr, er = out["pt_rows"].astype(np.int64), out["edge_rows"].astype(np.int64)
    assert pr.size > 0.5 * n_pt * cap / sum(a.nbytes for a in arrays.values()) and np.all(np.diff(pr) > 0) and np.all(np.diff(er) > 0)
    assert np.array_equal(out["pt_xyz"], arrays["pt_xyz"][pr]) and np.array_equal(out["chi2_per_edge"], arrays["chi2_per_edge"][er])
    assert np.array_equal(out["depth_positive"], arrays["depth_positive"][er]) and np.array_equal(out["cam_qt"], arrays["cam_qt"])
    again = bench.cap_outputs(arrays, cap)
    assert all(np.array_equal(again[k], out[k]) for k in out)
    small = bench.cap_outputs(arrays, 64 << 20)
    assert set(small) == set(arrays) and all(small[k] is arrays[k] for k in arrays)
