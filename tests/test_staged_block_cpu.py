"""The staged device block of the five map stages (csrc/staged_block.h, csrc/stage_blocks.h) on the CPU: tests/host/staged_block_check.cpp
rebuilds the five declarations at small counts (P = 0, NL = 0, cap = 0, K = 1, byte counts 0 / 1 / 3 / 4 / 5, odd word counts in front of the 8- and 16-byte-aligned
segments) and compares every offset and total with the formulas the wrappers held before, checks alignment and zeroed pads, fills every segment to its
declared length inside a malloc'd block of exactly the computed size, and has non-contiguous declarations rejected.  Built with the address and
undefined-behaviour sanitizers, so an overrun of the host block ends the program."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_staged_block_layouts_under_the_sanitizers(tmp_path):
    exe = tmp_path / "staged_block_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe), os.path.join(HERE, "host", "staged_block_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("staged block ok") and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
