"""smhip_shard --close-loops with --odom FILE: the odometry calibration factors of IsamOptimizer ("Odometry calibration
factor") on the 72-scan circle drive of test_close_loops_gpu.py, with an odometer made from the truth.  The refusals need no GPU."""
import json
import subprocess

import numpy as np
import pytest

from test_close_loops_gpu import LOOP_FLAGS, N_SCANS, PERIOD, RADIUS, circle_drive  # noqa: F401  (the fixture)

TF = (0.8, -0.2, 0.5, 0.01, -0.02, 0.3)                      # odom -> lidar: tx, ty, tz, rx, ry, rz
TF_OFF = (0.8, -0.2, 0.5, 0.01 + 0.06, -0.02 - 0.05, 0.3 + 0.0624)   # about 0.1 rad off


def transform(v):
    """common::Vector6ToTransform: the translation, then R = Rz(rz) Ry(ry) Rx(rx)"""
    tx, ty, tz, r, p, y = v
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = (tx, ty, tz)
    return T


def rotation_error(A, B):
    c = 0.5 * (np.trace(A[:3, :3].T @ B[:3, :3]) - 1.0)
    return float(np.arccos(np.clip(c, -1.0, 1.0)))


def write_odom(path, truth, lines=None, nan=()):
    """a line per scan: the odometer's pose tf truth_k tf^-1 behind an arbitrary first reading, as a row-major 3 x 4"""
    tf = transform(TF)
    first = transform((5.0, -3.0, 0.2, 0.0, 0.0, 1.0))
    with open(path, "w") as fh:
        for k, X in enumerate(truth[:len(truth) if lines is None else lines]):
            O = first @ tf @ X @ np.linalg.inv(tf)
            fh.write(" ".join(["nan"] * 12 if (nan == "all" or k in nan) else ["%.17g" % x for x in O[:3].ravel()]) + "\n")


@pytest.fixture(scope="module")
def exe():
    from staticmapping_amd import build
    build.build()
    return build.build_shard_driver()


def test_the_refusals_end_the_run_before_any_device_work(exe, tmp_path):
    scans = tmp_path / "scans"
    scans.mkdir()
    for k in range(3):
        (scans / ("%06d.bin" % k)).write_bytes(b"")
    truth = [np.eye(4)] * 3
    good = tmp_path / "odom.txt"
    write_odom(good, truth)

    def run(*flags, scans_dir=str(scans)):
        r = subprocess.run([exe, "--scans", scans_dir, *flags], capture_output=True, text=True, cwd=tmp_path)
        assert not (tmp_path / "x.txt").exists()
        return r
    r = run("--odom", str(good))
    assert r.returncode == 2 and "--odom needs --close-loops" in r.stderr
    for flags in (["--odom-calib"], ["--odom-tf", "0,0,0,0,0,0"], ["--odom-huber", "1"]):
        r = run("--close-loops", "x.txt", *flags)
        assert r.returncode == 2 and "need --odom" in r.stderr
    short = tmp_path / "short.txt"
    write_odom(short, truth, lines=2)
    r = run("--close-loops", "x.txt", "--odom", str(short))
    assert r.returncode == 2 and "holds 2 lines for 3 scans" in r.stderr
    for bad_line in ("1 0 0 0 0 1 0 0 0 0 1", "1 0 0 0 0 1 0 0 0 0 1 0 7", "1 0 0 0 0 1 0 zero 0 0 1 0"):
        bad = tmp_path / "bad.txt"
        bad.write_text(good.read_text().splitlines()[0] + "\n" + bad_line + "\n" + good.read_text().splitlines()[2] + "\n")
        r = run("--close-loops", "x.txt", "--odom", str(bad))
        assert r.returncode == 2 and "line 2 does not hold 12 numbers" in r.stderr
    r = run("--close-loops", "x.txt", "--odom", str(tmp_path / "missing.txt"))
    assert r.returncode == 2 and "cannot read" in r.stderr
    for tf in ("0,0,0,0,0", "0,0,0,0,0,0,0", "0,0,0,0,0,nan", "a,b,c,d,e,f", ""):
        r = run("--close-loops", "x.txt", "--odom", str(good), "--odom-tf", tf)
        assert r.returncode == 2 and "bad odometry setting" in r.stderr and "--odom-tf" in r.stderr
    for k in ("-1", "nan", "inf", "one", "1x", ""):
        r = run("--close-loops", "x.txt", "--odom", str(good), "--odom-huber", k)
        assert r.returncode == 2 and "bad odometry setting" in r.stderr and "--odom-huber" in r.stderr
    r = run("--no-such-flag")
    assert r.returncode == 2 and all(f in r.stderr for f in ("--odom ", "--odom-tf", "--odom-calib", "--odom-huber"))
    r = run("--close-loops", "x.txt", "--odom", str(good), "--odom-tf", "0.1,0,0,0,0,0.2", "--odom-calib", "--odom-huber", "2", scans_dir="/nonexistent-dir")
    assert r.returncode == 2 and "cannot open" in r.stderr            # every flag known and in order: it gets as far as the scans


@pytest.fixture(scope="module")
def drive_runs(circle_drive, exe, tmp_path_factory):  # noqa: F811
    """the driver on the circle drive, once per set of flags: run(tag, extra) -> (corrected pose file, JSON line), kept for the module"""
    from staticmapping_amd import kitti
    seq, poses = circle_drive
    tmp = tmp_path_factory.mktemp("odom_runs")
    truth = [np.linalg.inv(poses[0]) @ P for P in poses]
    step = 2.0 * np.pi * RADIUS / PERIOD
    common = ["--scans", seq, "--gpus", "1", "--batch", "8", "--iterations", "30", "--guess-tx", "%.4f" % step] + LOOP_FLAGS
    odom, nans = tmp / "odom.txt", tmp / "nan.txt"
    write_odom(odom, truth, nan=(4, 5, 6))                             # (a submap's reading is its first frame's: scan 6 is one)
    write_odom(nans, truth, nan="all")
    done = {}

    def run(tag, extra=()):
        if tag not in done:
            out, corrected = tmp / ("pose_%s.txt" % tag), tmp / ("corrected_%s.txt" % tag)
            r = subprocess.run([exe] + common + ["--out", str(out), "--close-loops", str(corrected)] + list(extra), capture_output=True, text=True, timeout=600)
            print(r.stderr[-1500:])
            assert r.returncode == 0, r.returncode
            done[tag] = (corrected, json.loads(r.stdout.strip().splitlines()[-1]))
        return done[tag]

    def to_truth(path):
        T = kitti.read_poses(str(path))
        return max(np.linalg.norm(T[k][:3, 3] - truth[k][:3, 3]) for k in range(N_SCANS))
    return dict(run=run, to_truth=to_truth, odom=str(odom), nans=str(nans))


TF_FLAG = "%.17g,%.17g,%.17g,%.17g,%.17g,%.17g"


@pytest.mark.gpu
def test_a_file_without_a_reading_changes_nothing(drive_runs):
    plain, line0 = drive_runs["run"]("plain")
    empty, line1 = drive_runs["run"]("nan", ["--odom", drive_runs["nans"]])
    assert "odom_factors" not in line0 and "odom_tf" not in line0
    assert empty.read_bytes() == plain.read_bytes() and line1["odom_factors"] == 0
    assert (np.array(line1["odom_tf"]).reshape(4, 4) == np.eye(4)).all() and set(line1) - set(line0) == {"odom_factors", "odom_tf"}


@pytest.mark.gpu
def test_odometry_bounds_the_drift(drive_runs):
    plain, _ = drive_runs["run"]("plain")
    held, line = drive_runs["run"]("odom", ["--odom", drive_runs["odom"], "--odom-tf", TF_FLAG % TF])
    assert line["odom_factors"] == N_SCANS // 3 - 1 and line["pose_graph_stop_reason"] in (1, 2)       # every submap but the one whose first scan is 6
    assert np.abs(np.array(line["odom_tf"]).reshape(4, 4) - transform(TF)).max() < 1e-12               # held: reported as given
    e0, e1 = drive_runs["to_truth"](plain), drive_runs["to_truth"](held)
    print("worst distance to the truth: %.4f m without --odom, %.4f m with it" % (e0, e1))
    assert e1 < e0


@pytest.mark.gpu
def test_the_calibration_is_found_from_a_start_a_tenth_of_a_radian_off(drive_runs):
    free, line = drive_runs["run"]("calib", ["--odom", drive_runs["odom"], "--odom-tf", TF_FLAG % TF_OFF, "--odom-calib"])
    r0, r1 = rotation_error(transform(TF_OFF), transform(TF)), rotation_error(np.array(line["odom_tf"]).reshape(4, 4), transform(TF))
    print("rotation error of odom_tf: %.4f rad given, %.4f rad reported; worst distance to the truth %.4f m" % (r0, r1, drive_runs["to_truth"](free)))
    assert line["odom_factors"] == N_SCANS // 3 - 1 and 0.08 < r0 < 0.12
    assert r1 < r0
