"""The staged device block (csrc/staged_block.h, csrc/stage_blocks.h) on the CPU, for ten declarations: the five map stages declared first and the
five blocks of six entry points of hamming.hip and frame.hip (dense, CSR single and multi on one block, BoW transform, frustum, normal and depth).
tests/host/staged_block_check.cpp rebuilds the declarations at small counts (P = 0, NL = 0, cap = 0, K = 1, T = 0, n_cand = 0, byte counts 0 / 1 / 3 / 4 / 5,
an odd number of 16-bit distances, odd word counts in front of the 8- and 16-byte-aligned segments, every optional output asked for and not) and compares every
offset and total with the formulas the wrappers held before, checks alignment and zeroed pads, that a zero-element segment takes no room, fills every segment to its
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
