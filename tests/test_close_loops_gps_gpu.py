"""smhip_shard --close-loops OUT --gps-enu FILE on the drive of test_close_loops_gpu.py (72 scans of 10 000 points once round a 12 m
circle and on), FILE made from the truth: a line per scan, the antenna's place in an ENU frame 350 m away and turned by 0.4 rad.  The
driver's own poses drift by tens of metres on this drive and no loop is ever seen, so the GPS factors are all that bounds the drift."""
import json
import subprocess

import numpy as np
import pytest

import pose_graph_gps_ref as gps
import pose_graph_ref as ref
from test_close_loops_gpu import LOOP_FLAGS, N_SCANS, PERIOD, RADIUS, circle_drive  # noqa: F401  (the fixture)

FRAME = ref.make_pose((0.01, -0.02, 0.4), (350.0, -120.0, 12.0))
LEVER = np.array([0.3, -0.2, 1.1])
INIT_NUM = 10                           # 24 submaps: the default 25 would cache every fix and never add a factor


def test_gps_enu_needs_close_loops_and_a_line_per_scan(tmp_path):
    """both end with exit 2 before any device work"""
    from staticmapping_amd import build
    build.build()
    exe = build.build_shard_driver()
    for k in range(3):
        np.zeros((2, 4), np.float32).tofile(str(tmp_path / ("%06d.bin" % k)))
    enu = tmp_path / "enu.txt"
    enu.write_text("1 2 3\nnan nan nan\n")
    r = subprocess.run([exe, "--scans", str(tmp_path), "--gps-enu", str(enu)], capture_output=True, text=True)
    assert r.returncode == 2 and "--gps-enu needs --close-loops" in r.stderr
    r = subprocess.run([exe, "--scans", str(tmp_path), "--close-loops", str(tmp_path / "o.txt"), "--gps-enu", str(enu)], capture_output=True, text=True)
    assert r.returncode == 2 and "holds 2 lines for 3 scans" in r.stderr
    assert not (tmp_path / "o.txt").exists()
    r = subprocess.run([exe, "--scans", str(tmp_path), "--close-loops", str(tmp_path / "o.txt"), "--gps-output-enu"], capture_output=True, text=True)
    assert r.returncode == 2 and "--gps-output-enu needs --gps-enu" in r.stderr
    r = subprocess.run([exe, "--scans", str(tmp_path), "--close-loops", str(tmp_path / "o.txt"), "--gps-enu", str(enu), "--gps-lever", "1,2"], capture_output=True, text=True)
    assert r.returncode == 2 and "--gps-lever takes x,y,z" in r.stderr


def kabsch(P, Q):
    """the rigid (R, t) that brings the points P closest to Q"""
    cp, cq = P.mean(axis=0), Q.mean(axis=0)
    U, _, Vt = np.linalg.svd((P - cp).T @ (Q - cq))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    return R, cq - R @ cp


@pytest.mark.gpu
def test_gps_factors_put_the_drive_into_the_enu_frame(circle_drive, tmp_path):
    from staticmapping_amd import build, kitti
    seq, poses = circle_drive
    exe = build.build_shard_driver()
    step = 2.0 * np.pi * RADIUS / PERIOD
    common = ["--scans", seq, "--gpus", "1", "--batch", "8", "--iterations", "30", "--guess-tx", "%.4f" % step] + LOOP_FLAGS
    truth = np.stack([np.linalg.inv(poses[0]) @ P for P in poses])              # the map frame: scan 0 at the identity
    enu = np.stack([FRAME[:3, :3] @ (T[:3, :3] @ LEVER + T[:3, 3]) + FRAME[:3, 3] for T in truth])
    enu_file, nan_file = tmp_path / "enu.txt", tmp_path / "nan.txt"
    np.savetxt(enu_file, enu, fmt="%.17g")
    nan_file.write_text("nan nan nan\n" * N_SCANS)

    def run(tag, extra):
        out, corrected = tmp_path / ("pose_%s.txt" % tag), tmp_path / ("corrected_%s.txt" % tag)
        r = subprocess.run([exe] + common + ["--out", str(out), "--close-loops", str(corrected)] + extra, capture_output=True, text=True, timeout=600)
        print(r.stderr[-1500:])
        assert r.returncode == 0, r.returncode
        return corrected, json.loads(r.stdout.strip().splitlines()[-1])
    gps_flags = ["--gps-lever", ",".join("%.17g" % x for x in LEVER), "--gps-init-num", str(INIT_NUM)]
    plain, line0 = run("plain", [])
    with_gps, line1 = run("gps", ["--gps-enu", str(enu_file), "--gps-output-enu"] + gps_flags)
    with_nan, line2 = run("nan", ["--gps-enu", str(nan_file)] + gps_flags)
    # without the flag no new field; with it, two
    assert not [k for k in line0 if "gps" in k]
    assert {k for k in line1 if k not in line0} == {"gps_factors", "gps_coord"}
    # a FILE of all nan: the pose file of the run without the flag, byte for byte, and no factor
    assert with_nan.read_bytes() == plain.read_bytes()
    assert line2["gps_factors"] == 0 and line2["gps_coord"] == list(np.eye(4).ravel())
    # the factor count is the restated rule's for the 24 submaps: the angle (0.3 rad a submap) is there long before the tenth fix
    S = N_SCANS // 3
    before = kitti.read_poses(str(plain))
    angles = [gps.max_rotation(list(before[0:3 * k + 1:3])) for k in range(S)]
    rule = gps.gps_rule([True] * S, angles, init_num=INIT_NUM)
    print("rule", rule, "angles", angles[:INIT_NUM + 1])
    assert angles[INIT_NUM] > 1.6 + 0.5                                          # (far from the threshold: the proxy poses cannot decide otherwise)
    assert rule["trigger"] == INIT_NUM and line1["gps_factors"] == len(rule["factors"]) == S - 1
    G = np.array(line1["gps_coord"]).reshape(4, 4)
    assert np.abs(G[:3, :3].T @ G[:3, :3] - np.eye(3)).max() < 1e-12 and np.linalg.det(G[:3, :3]) > 0 and (G[3] == [0, 0, 0, 1]).all()
    # OUT is in the ENU frame: every frame closer to the truth's ENU position than the run without GPS gets after a best rigid fit
    want = np.stack([(FRAME @ T)[:3, 3] for T in truth])
    got = kitti.read_poses(str(with_gps))[:, :3, 3]
    R, t = kabsch(before[:, :3, 3], want)
    fitted = before[:, :3, 3] @ R.T + t
    err_gps, err_fit = np.linalg.norm(got - want, axis=1).max(), np.linalg.norm(fitted - want, axis=1).max()
    print("largest distance to the truth's ENU positions: %.3f m with GPS factors, %.3f m without after a best rigid fit" % (err_gps, err_fit))
    print("gps_coord", G, "off the truth frame by", np.linalg.norm(G[:3, 3] - FRAME[:3, 3]), np.linalg.norm(ref.log_so3(FRAME[:3, :3].T @ G[:3, :3])))
    assert err_gps < err_fit
