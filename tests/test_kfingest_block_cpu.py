"""KfIngestBlock, the staged device block of ccm_kfstore_ingest (csrc/stage_blocks.h), and the host side of csrc/kfingest_math.h on the CPU:
tests/host/kfingest_block_check.cpp declares the block at small counts (F = 0 and M = 1 among them, the per-feature outputs absent and present), checks every
offset and both copied ranges, and fills every segment to its declared length inside a malloc'd block of exactly the computed size; it also runs the descent, the
argument rules and the sequential evaluator on rows whose answer is certain, on arrays of exactly the documented lengths.  Built with the address and
undefined-behaviour sanitizers as a stand-alone program and run as a child process, so an overrun of the host block ends the program."""
import os
import subprocess

from ccm_slam_amd import kfstore  # noqa: F401  (the block is the store's)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_kfingest_block_layout_and_evaluator_under_the_sanitizers(tmp_path):
    exe = tmp_path / "kfingest_block_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe), os.path.join(HERE, "host", "kfingest_block_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("kfingest block ok") and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
