"""KfstoreAddBlock, FuseSim3ResidentBlock and FusePoseResidentBlock, the staged device blocks of ccm_kfstore_add and of the two resident Fuse calls
(csrc/stage_blocks.h), on the CPU: tests/host/kfstore_block_check.cpp declares them at the sizes of the GPU tests (a keyframe without features,
a supplied grid and none, uv absent and present among them), checks every offset and both copied ranges, and fills every segment to its declared length inside a
malloc'd block of exactly the computed size; it also runs the host grid build and the add rules of csrc/kfstore_math.h on arrays of exactly
the documented lengths.  Built with the address and undefined-behaviour sanitizers as a stand-alone program and run as a child process, so an
overrun of the host block ends the program."""
import os
import subprocess

from ccm_slam_amd import kfstore  # noqa: F401  (the blocks are the store's)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_kfstore_block_layouts_under_the_sanitizers(tmp_path):
    exe = tmp_path / "kfstore_block_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "ccm_slam_amd", "csrc"), "-o", str(exe), os.path.join(HERE, "host", "kfstore_block_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("kfstore blocks ok") and not r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
