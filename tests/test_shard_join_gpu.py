"""smhip_shard --save-trajectory-map and the join mode: the 72-scan circle drive of tests/test_close_loops_gpu.py goes through
--close-loops once and is saved as map A; B is A displaced by 0.5 m and 0.5 degrees, written here; the join with the base held gives C.
Without the new flags every output of the driver is what it was, byte for byte."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

N_SCANS, PERIOD, RADIUS = 72, 63, 12.0
LOOP_FLAGS = ["--submap-frames", "3", "--loop-ignore-threshold", "6", "--loop-max-distance", "5", "--loop-use-descriptor", "0"]
SUBMAPS = N_SCANS // 3


def _exe():
    from staticmapping_amd import build
    build.build()
    return build.build_shard_driver()


def test_the_join_flags_are_parsed_and_refused(tmp_path):
    """no device: every refusal ends the run with exit 2 before any device work"""
    exe = _exe()

    def refused(args, words):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and words in r.stderr, (args, r.returncode, r.stderr)
    refused(["--join-base", "a.xml"], "a join takes --join-base, --join-incremental and --join-out together")
    refused(["--join-base", "a.xml", "--join-out", "c.xml"], "a join takes --join-base, --join-incremental and --join-out together")
    join = ["--join-base", "a.xml", "--join-incremental", "b.xml", "--join-out", "c.xml"]
    refused(join + ["--scans", "/nonexistent-dir"], "a join is a run of its own")
    refused(join + ["--save-trajectory-map", "x"], "a join takes no")
    refused(join + ["--join-connection-huber", "-1"], "bad join setting")
    refused(join + ["--join-connection-huber", "1x"], "bad join setting")
    refused(join + ["--loop-huber", "nan"], "bad loop setting")
    refused(["--scans", "/nonexistent-dir", "--join-hold-base", "1"], "need --join-base, --join-incremental and --join-out")
    refused(["--scans", "/nonexistent-dir", "--join-pcd", "x.pcd"], "need --join-base, --join-incremental and --join-out")
    refused(["--scans", "/nonexistent-dir", "--save-trajectory-map", "x"], "--save-trajectory-map needs --close-loops")
    refused(["--join-hold-base", "1"], "need --join-base, --join-incremental and --join-out")
    # every flag known: the run gets as far as the base map's file, and its reader's reason ends it
    refused(join + ["--join-hold-base", "1", "--join-connection-huber", "1", "--join-pcd", "w.pcd", "--join-static-map", "s.pcd", "--loop-huber", "1",
                    "--loop-report", "r.txt", "--loop-max-distance", "5"], "map file does not exist: a.xml")
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trajectory_map", "two_trajectories.xml")
    refused(["--join-base", golden, "--join-incremental", str(tmp_path / "none.xml"), "--join-out", str(tmp_path / "c.xml")], "map file does not exist: " + str(tmp_path / "none.xml"))
    bad = tmp_path / "bad.xml"
    bad.write_text(open(golden).read().replace("t0_s1.bin", "gone.bin"))
    refused(["--join-base", str(bad), "--join-incremental", golden, "--join-out", str(tmp_path / "c.xml")], "submap file does not exist")


@pytest.fixture(scope="module")
def circle_drive(tmp_path_factory):
    """the drive of tests/test_close_loops_gpu.py: once round a circle and on over its first nine scans"""
    from staticmapping_amd import kitti, synth
    d = tmp_path_factory.mktemp("circle")
    poses = []
    for k in range(N_SCANS):
        a = 2.0 * np.pi * k / PERIOD
        poses.append(synth.make_pose(t=(RADIUS * np.sin(a), RADIUS * (1.0 - np.cos(a)), 0.0), rpy_deg=(0, 0, np.rad2deg(a))))
    scene = synth.make_drive_scene(poses, seed=7)
    for k, P in enumerate(poses):
        kitti.write_bin(kitti.scan_path(str(d), k), synth.velodyne_scan(synth.scene_near(scene, P[:3, 3]), P, seed=2000 + k, n_points=10_000))
    return str(d), poses


def vector6_to_transform(v):
    tx, ty, tz, rx, ry, rz = v
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    X = np.eye(4)
    X[:3, :3] = Rz @ Ry @ Rx
    X[:3, 3] = tx, ty, tz
    return X


def transform_to_vector6(X):
    R = X[:3, :3]
    sy = np.hypot(R[0, 0], R[1, 0])
    return [X[0, 3], X[1, 3], X[2, 3], np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], sy), np.arctan2(R[1, 0], R[0, 0])]


SUBMAP = re.compile(r'<Submap id="(\d+)" file="([^"]*)" tx="([^"]*)" ty="([^"]*)" tz="([^"]*)" rx="([^"]*)" ry="([^"]*)" rz="([^"]*)" connections="([^"]*)" />')


def submaps_of(trajectory_text):
    return [dict(id=int(m[0]), file=m[1], pose=vector6_to_transform([float(x) for x in m[2:8]]), connections=m[8]) for m in SUBMAP.findall(trajectory_text)]


@pytest.mark.gpu
def test_a_saved_map_joins_a_displaced_copy_of_itself(circle_drive, tmp_path):
    from staticmapping_amd import synth
    seq, _ = circle_drive
    exe = _exe()
    step = 2.0 * np.pi * RADIUS / PERIOD
    common = ["--scans", seq, "--gpus", "1", "--batch", "8", "--iterations", "30", "--guess-tx", "%.4f" % step]
    A = tmp_path / "A"

    def run(tag, extra):
        out, edges, corrected = tmp_path / ("pose_%s.txt" % tag), tmp_path / ("edges_%s.txt" % tag), tmp_path / ("corrected_%s.txt" % tag)
        r = subprocess.run([exe] + common + ["--out", str(out), "--submap-edges", str(edges), "--close-loops", str(corrected)] + LOOP_FLAGS + extra,
                           capture_output=True, text=True, timeout=600)
        print(r.stderr[-1500:])
        assert r.returncode == 0, r.returncode
        return out, edges, corrected, json.loads(r.stdout.strip().splitlines()[-1])
    # run 1, with and without the new flag: every other output is the same, byte for byte, and the line gains nothing
    plain, saved = run("plain", []), run("saved", ["--save-trajectory-map", str(A)])
    for a, b in zip(plain[:3], saved[:3]):
        assert a.read_bytes() == b.read_bytes()
    timing = {k for k in plain[3] if k.endswith("seconds") or k.endswith("_s") or k.endswith("_s_rank0") or k.endswith("_file")}
    assert set(plain[3]) == set(saved[3]) and {k: v for k, v in plain[3].items() if k not in timing} == {k: v for k, v in saved[3].items() if k not in timing}
    # A: one trajectory, a cloud file per submap, each submap connected to the next (and to the sources of its loop edges)
    a_text = (A / "map.xml").read_text()
    assert a_text.count("<Trajectory ") == 1 and 'id="0" enu_x="0" enu_y="0"' in a_text
    a_maps = submaps_of(a_text)
    assert [s["id"] for s in a_maps] == list(range(SUBMAPS)) and [s["file"] for s in a_maps] == ["submap_%d.bin" % k for k in range(SUBMAPS)]
    for k, s in enumerate(a_maps):
        assert s["connections"].startswith("[0,%d]" % (k + 1)) if k + 1 < SUBMAPS else "[0,%d]" % (k + 1) not in s["connections"]
        size = (A / s["file"]).stat().st_size
        assert size > 20 + 20 * 1000 and (size - 20) % 20 == 0
    assert sum(s["connections"].count("[") for s in a_maps) == SUBMAPS - 1 + saved[3]["loop_edges"]
    # the poses are the corrected ones: the first frame of every submap in the corrected file
    from staticmapping_amd import kitti
    corrected = kitti.read_poses(str(saved[2]))
    assert max(np.abs(a_maps[k]["pose"] - corrected[3 * k]).max() for k in range(SUBMAPS)) < 1e-5        # (that file carries 8 significant digits)

    # B: A's map.xml with every pose premultiplied by the drift, the cloud files copied
    B = tmp_path / "B"
    B.mkdir()
    drift = synth.make_pose(t=(0.3, 0.4, 0.0), rpy_deg=(0, 0, 0.5))
    for s in a_maps:
        shutil.copy(A / s["file"], B / s["file"])

    def displaced(m):
        v = transform_to_vector6(drift @ vector6_to_transform([float(x) for x in m.groups()[2:8]]))
        return '<Submap id="%s" file="%s" tx="%.17g" ty="%.17g" tz="%.17g" rx="%.17g" ry="%.17g" rz="%.17g" connections="%s" />' % ((m[1], m[2]) + tuple(v) + (m[9],))
    (B / "map.xml").write_text(SUBMAP.sub(displaced, a_text))
    b_maps = submaps_of((B / "map.xml").read_text())

    # run 2: the join with the base held; C is written beside A's files, so trajectory 0 keeps their names
    C, pcd, static, report = A / "joined.xml", tmp_path / "whole.pcd", tmp_path / "static.pcd", tmp_path / "cross_edges.txt"
    r = subprocess.run([exe, "--join-base", str(A / "map.xml"), "--join-incremental", str(B / "map.xml"), "--join-out", str(C), "--join-hold-base", "1",
                        "--join-pcd", str(pcd), "--join-static-map", str(static), "--loop-report", str(report)] + LOOP_FLAGS[2:], capture_output=True, text=True, timeout=600)
    print(r.stderr[-1500:])
    assert r.returncode == 0, r.returncode
    line = json.loads(r.stdout.strip().splitlines()[-1])
    print(line)
    assert line["join_base_submaps"] == SUBMAPS and line["join_incremental_submaps"] == SUBMAPS and line["join_loop_edges"] >= 2
    assert line["join_pose_graph_stop_reason"] in (1, 2) and line["join_pcg_iterations"] >= 1 and line["join_solve_seconds"] > 0.0
    c_text = C.read_text()
    parts = c_text.split("<Trajectory ")
    assert len(parts) == 3 and parts[1].startswith('id="0"') and parts[2].startswith('id="1"')
    # trajectory 0 is A's text exactly, apart from the "[1,k]" entries added to its connection strings
    c0 = "<Trajectory " + parts[1]
    a0 = "<Trajectory " + a_text.split("<Trajectory ")[1].split("</Trajectory>")[0] + "</Trajectory>\n"
    added = re.findall(r"\[1,\d+\]", c0)
    assert len(added) == line["join_loop_edges"] and re.sub(r"\[1,\d+\]", "", c0).rstrip("\t") == a0.rstrip("\t")
    edges = [[float(x) for x in row.split()] for row in report.read_text().splitlines()]
    assert len(edges) == line["join_loop_edges"] and all(t < SUBMAPS <= s for t, s, _, _ in edges)
    with_edge = sorted({int(s) - SUBMAPS for _, s, _, _ in edges})
    assert sorted(int(x[3:-1]) for x in added) == sorted(int(s) - SUBMAPS for _, s, _, _ in edges)
    # the 0.5 bound at B's submaps that got an edge, against A's poses of the same submap
    c1 = submaps_of(parts[2])
    assert [s["file"] for s in c1] == [str(B / ("submap_%d.bin" % k)) for k in range(SUBMAPS)]          # files elsewhere are named by their full path
    for k in with_edge:
        before = np.linalg.norm(b_maps[k]["pose"][:3, 3] - a_maps[k]["pose"][:3, 3])
        after = np.linalg.norm(c1[k]["pose"][:3, 3] - a_maps[k]["pose"][:3, 3])
        print("submap %d: %.3f m from A's as loaded, %.3f m after, factor %.3f" % (k, before, after, after / before))
        assert after < 0.5 * before
    assert line["join_pcd_points"] > 1000 and line["join_static_map_voxels"] > 1000
    for f in (pcd, static):
        head = open(f, "rb").read(400).decode("ascii", "replace")
        assert int(head.split("POINTS ")[1].split("\n")[0]) > 1000
