"""TriSearchResidentBlock, the staged device block of ccm_tri_search_eval_resident (csrc/stage_blocks.h), and the lines of csrc/tri_search_math.h
on the CPU: tests/host/tri_search_block_check.cpp checks every offset and both copied ranges and fills every segment to its declared length inside a malloc'd block
of exactly the computed size; it holds tsm_accept and tsm_merge to the sequential loop on every list of up to five (distance, gate) pairs over the distances
{0, 1, 50, 51} at every split point and every pair of split points, and takes the word packing through its round trip (index 65 534 among the values).  Built with
the address and undefined-behaviour sanitizers as a stand-alone program and run as a child process, so an overrun of the host block ends the program."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_tri_search_block_layout_and_lines_under_the_sanitizers(tmp_path):
    exe = tmp_path / "tri_search_block_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe), os.path.join(HERE, "host", "tri_search_block_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("tri_search block ok") and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
