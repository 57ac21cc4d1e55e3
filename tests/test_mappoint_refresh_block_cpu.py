"""MapPointRefreshBlock, the staged device block of ccm_mappoint_refresh_resident (csrc/stage_blocks.h), and the lines of csrc/mappoint_math.h on
the CPU: tests/host/mappoint_refresh_block_check.cpp checks every offset and both copied ranges and fills every segment to its declared length inside a malloc'd
block of exactly the computed size, with and without the normal / depth segments and the winners' descriptors; it holds mpm_select to a literal sort on every row of
up to six distances over {0, 1, 255, 256} at every rank, and runs the host evaluator of one point on rows whose answer is certain.  Built with the address and
undefined-behaviour sanitizers as a stand-alone program and run as a child process, so an overrun of the host block ends the program."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_mappoint_refresh_block_layout_and_lines_under_the_sanitizers(tmp_path):
    exe = tmp_path / "mappoint_refresh_block_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe), os.path.join(HERE, "host", "mappoint_refresh_block_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("mappoint_refresh block ok") and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
