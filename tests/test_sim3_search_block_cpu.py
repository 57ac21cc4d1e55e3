"""Sim3ProjectResidentBlock and Sim3PairResidentBlock, the staged device blocks of ccm_sim3_project_eval_resident and ccm_sim3_pair_eval_resident
(csrc/stage_blocks.h), on the CPU: tests/host/sim3_search_block_check.cpp declares them at the sizes of the GPU tests (a keyframe without
features, mask lengths that are no multiple of four, an empty job, uv absent and present among them), checks every offset and both copied ranges, and fills every
segment to its declared length inside a malloc'd block of exactly the computed size.  Built with the address and undefined-behaviour sanitizers as a stand-alone
program and run as a child process, so an overrun of the host block ends the program."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_sim3_search_block_layouts_under_the_sanitizers(tmp_path):
    exe = tmp_path / "sim3_search_block_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe), os.path.join(HERE, "host", "sim3_search_block_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("sim3_search blocks ok") and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
