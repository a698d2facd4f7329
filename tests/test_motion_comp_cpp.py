"""The header's host form of the motion compensation (include/smhip/front_end.h: MotionCompensation, InterpolateTransform,
AverageTransforms) against the numpy restatement (tests/motion_comp_ref.py), without a GPU.

Every float coordinate within 1 ulp and at most 1e-4 of them different at all: two correctly implemented double sin / acos differ
by a few double ulps, which moves a coordinate by ~1e-13 m and changes the float only when the double lies that close to a
rounding boundary -- then by exactly 1 ulp; the cap keeps a wrong formula from hiding behind "1 ulp"."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_motion_compensation.cc")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_comp_ref as mc  # noqa: E402


def _build_exe():
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_motion_compensation")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    hdrs = [os.path.join(ROOT, "include", "smhip", h) for h in ("front_end.h", "back_end.h", "registrator.h")] + [os.path.join(ROOT, "include", "smhip.h")]
    if (not os.path.exists(exe)) or max([os.path.getmtime(SRC), os.path.getmtime(lib)] + [os.path.getmtime(h) for h in hdrs]) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                               "-L", os.path.dirname(lib), "-lsmhip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def _scan(n=120_000, seed=5):
    """a Velodyne-like cloud of the seeded drive with the collector's factors i / n"""
    from staticmapping_amd import synth
    rows4 = synth.velodyne_scan(synth.make_scene(0), synth.make_pose(), seed=seed, n_points=n)
    rows = np.zeros((len(rows4), 5), np.float32)
    rows[:, :4] = rows4[:, :4]
    rows[:, 4] = (np.arange(len(rows), dtype=np.float64) / len(rows)).astype(np.float32)
    return rows


@pytest.fixture(scope="module")
def scan():
    return _scan()


def test_header_compiles_with_warnings_on():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), SRC])


@pytest.mark.parametrize("name", ["drive", "half_turn", "tiny", "identity"])
def test_motion_compensation_matches_the_restatement(name, scan, tmp_path):
    assert len(scan) == 120_000
    delta = mc.check_deltas()[name]
    scan.tofile(tmp_path / "rows.bin")
    np.ascontiguousarray(delta.T).tofile(tmp_path / "delta.bin")              # column-major
    subprocess.check_call([_build_exe(), "compensate", str(tmp_path / "rows.bin"), str(tmp_path / "delta.bin"), str(tmp_path / "out.bin")], timeout=120)
    got = np.fromfile(tmp_path / "out.bin", np.float32).reshape(-1, 5)
    want = mc.motion_compensation(scan, delta)
    assert got.shape == want.shape
    assert got[:, 3:].tobytes() == scan[:, 3:].tobytes()                       # intensity and factor carried bit for bit
    mc.assert_one_ulp(got[:, :3], want[:, :3], "header MotionCompensation, " + name)
    if name != "identity":
        assert np.abs(got[:, :3] - scan[:, :3]).max() > 1e-3                   # it did move the cloud


@pytest.mark.parametrize("name", ["drive", "half_turn", "tiny", "identity"])
def test_interpolate_transform_matches_the_restatement(name, tmp_path):
    delta = mc.check_deltas()[name]
    np.ascontiguousarray(delta.T).tofile(tmp_path / "delta.bin")
    for f in (0.0, 0.3, 1.0):
        out = subprocess.check_output([_build_exe(), "interpolate", str(tmp_path / "delta.bin"), repr(f)], text=True, timeout=60)
        got = np.array([float(v) for v in out.split()]).reshape(4, 4)
        assert np.abs(got - mc.interpolate_transform(delta, f)).max() <= 1e-15


def test_average_transforms_matches_the_restatement(tmp_path):
    d = mc.check_deltas()
    for names in (("drive", "identity"), ("drive", "half_turn", "tiny"), ("half_turn",)):
        Ts = [d[k] for k in names]
        np.concatenate([np.ascontiguousarray(T.T).ravel() for T in Ts]).tofile(tmp_path / "t.bin")
        out = subprocess.check_output([_build_exe(), "average", str(tmp_path / "t.bin")], text=True, timeout=60)
        got = np.array([float(v) for v in out.split()]).reshape(4, 4)
        assert np.abs(got - mc.average_transforms(Ts)).max() <= 1e-15, names


def test_a_factor_outside_the_unit_interval_aborts_like_the_reference(scan, tmp_path):
    rows = scan[:100].copy()
    rows[17, 4] = 1.5
    rows.tofile(tmp_path / "rows.bin")
    np.eye(4).tofile(tmp_path / "delta.bin")
    r = subprocess.run([_build_exe(), "compensate", str(tmp_path / "rows.bin"), str(tmp_path / "delta.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "CHECK(factor >= 0. && factor <= 1.)" in r.stderr
