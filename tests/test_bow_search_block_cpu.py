"""BowPairResidentBlock, the staged device block of ccm_bow_pair_eval_resident (csrc/stage_blocks.h), and the lines of csrc/bow_search_math.h on
the CPU: tests/host/bow_search_block_check.cpp checks every offset and both copied ranges and fills every segment to its declared length inside a malloc'd block of
exactly the computed size; it holds bsm_update and bsm_merge to the sequential loop on every list of up to five distances over {0, 1, 2, 256} at every split point,
and takes the word packing through its round trip (index 65 534 and distance 256 among the values).  Built with the address and undefined-behaviour sanitizers as a
stand-alone program and run as a child process, so an overrun of the host block ends the program."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_bow_search_block_layout_and_lines_under_the_sanitizers(tmp_path):
    exe = tmp_path / "bow_search_block_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe), os.path.join(HERE, "host", "bow_search_block_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("bow_search block ok") and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
