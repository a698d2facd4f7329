"""include/smhip/sweep_motion.h without a GPU and without the library: tests/cpp/test_sweep_motion.cc compiles with plain g++, writes
the poses it is given as the pose writer does (8 significant digits), reads them back and prints smhip::SweepMotions of them; the
motions are compared with the numpy restatement (tests/map_compensation_ref.py) on the file as written."""
import os
import subprocess

import numpy as np
import pytest

import map_compensation_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_sweep_motion.cc")
HEADERS = [os.path.join(ROOT, "include", "smhip", "sweep_motion.h"), os.path.join(ROOT, "staticmapping_amd", "csrc", "shard_poses.h")]


def _build_exe():
    """no include path and nothing to link: both headers stand on the standard library alone"""
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_sweep_motion")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if (not os.path.exists(exe)) or max([os.path.getmtime(SRC)] + [os.path.getmtime(h) for h in HEADERS]) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", exe])
    return exe


@pytest.mark.parametrize("n", [1, 2, 9])
def test_sweep_motions_equal_the_restatement_on_the_file_as_written(n, tmp_path):
    from staticmapping_amd import kitti, synth
    world = np.asarray(synth.drive_poses(n, seed=5, speed=8.0, hz=10.0, yaw_rate_max=0.2))
    exact = np.stack([np.linalg.inv(world[0]) @ P for P in world])
    exact[:, :3, 3] += np.array([1234.56789012, -987.654321098, 12.3456789012])            # (so that 8 digits cut the translations)
    src, out = tmp_path / "exact.txt", tmp_path / "written.txt"
    with open(src, "w") as f:
        for P in exact:
            f.write(" ".join("%.17g" % v for v in P[:3, :].reshape(12)) + "\n")
    r = subprocess.run([_build_exe(), str(src), str(out)], text=True, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "all checks passed" and len(lines) == n + 1
    got = np.array([[float(v) for v in ln.split()] for ln in lines[:-1]]).reshape(n, 4, 4).transpose(0, 2, 1)   # column-major lines
    # the file holds 8 significant digits, and what is parsed back is exactly that
    written = kitti.read_poses(str(out))
    assert written.shape == (n, 4, 4)
    want8 = np.array([float("%.8g" % v) for v in exact[:, :3, :].reshape(-1)]).reshape(n, 3, 4)
    assert np.array_equal(written[:, :3, :], want8)
    assert not np.array_equal(written, exact)
    want = ref.sweep_motions(written)
    assert np.abs(got - want).max() <= 1e-12
    if n == 1:
        assert np.array_equal(got[0], np.eye(4))
    else:
        assert np.array_equal(got[-1], got[-2])                                   # the last frame repeats its predecessor's motion
        # and a motion is the step between two poses of the file.  (R^T, -R^T t) inverts a rotation block written with 8 digits only
        # as far as that block is orthonormal: entries off by <= 5e-9 leave R R^T within 3 * 2 * 5e-9 = 3e-8 of I, on a step below 1 m
        k = n - 2
        assert np.abs(written[k] @ got[k] - written[k + 1]).max() < 1e-7
