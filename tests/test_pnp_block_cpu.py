"""PnpRansacBlock, the staged device block of ccm_pnp_ransac_eval (csrc/stage_blocks.h), on the CPU: tests/host/pnp_block_check.cpp declares
it at the sizes of the GPU tests (one and several candidates, N around the 32-bit mask words, one hypothesis and a whole workgroup and one more), checks every offset
(the f64 intrinsics and poses stand on 8 bytes) and both copied ranges, and fills every segment to its declared length inside a malloc'd block of exactly the computed
size.  Built with the address and undefined-behaviour sanitizers as a stand-alone program and run as a child process, so an overrun of the host block ends the program."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_pnp_block_layout_under_the_sanitizers(tmp_path):
    exe = tmp_path / "pnp_block_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe), os.path.join(HERE, "host", "pnp_block_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("pnp block ok") and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
