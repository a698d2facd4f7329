"""staticmapping_amd/csrc/shard_poses.h without a GPU and without the library: tests/cpp/test_shard_poses.cc compiles with plain g++
and checks the driver's pose chain bit for bit against the row-major product, MulPose x AffineInverse, the pose file's write -> read
-> write trip and where ReadPoses stops."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_shard_poses.cc")
HEADER = os.path.join(ROOT, "staticmapping_amd", "csrc", "shard_poses.h")


def _build_exe():
    """no include path and nothing to link: the header stands on the standard library alone"""
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_shard_poses")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if (not os.path.exists(exe)) or max(os.path.getmtime(SRC), os.path.getmtime(HEADER)) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", exe])
    return exe


def test_pose_chain_pose_file_and_short_lines(tmp_path):
    out = subprocess.run([_build_exe(), str(tmp_path)], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
