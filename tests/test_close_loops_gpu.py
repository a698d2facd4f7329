"""smhip_shard --close-loops: a generated drive once round a circle and on over its first nine scans -> kitti_pose.txt -> submaps of three
scans, their descriptors and matches, IsamOptimizer with the loop detector after every submap -> the frames' poses in the pose
writer's format.  Without the flag every output is what it was, byte for byte; --map-poses on the corrected file builds a map."""
import json
import os
import subprocess

import numpy as np
import pytest

N_SCANS, PERIOD, RADIUS = 72, 63, 12.0
LOOP_FLAGS = ["--submap-frames", "3", "--loop-ignore-threshold", "6", "--loop-max-distance", "5", "--loop-use-descriptor", "0"]


def test_the_flag_is_parsed_and_refused_with_map_poses():
    from staticmapping_amd import build
    build.build()
    exe = build.build_shard_driver()
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", "x.txt", "--map", "m.pcd", "--map-poses", "p.txt"], capture_output=True, text=True)
    assert r.returncode == 2 and "--close-loops needs the alignment run" in r.stderr
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", "x.txt", "--loop-history", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "bad loop setting" in r.stderr
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", "x.txt", "--loop-m2dp-score", "0.98", "--loop-accept-score", "0.7",
                        "--loop-detect-count", "1", "--loop-max-z", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and "cannot open" in r.stderr            # every flag known: it gets as far as the scans


@pytest.fixture(scope="module")
def circle_drive(tmp_path_factory):
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


@pytest.mark.gpu
def test_close_loops_writes_corrected_frame_poses_and_leaves_the_rest_alone(circle_drive, tmp_path):
    from staticmapping_amd import build, kitti
    seq, poses = circle_drive
    exe = build.build_shard_driver()
    step = 2.0 * np.pi * RADIUS / PERIOD
    common = ["--scans", seq, "--gpus", "1", "--batch", "8", "--iterations", "30", "--guess-tx", "%.4f" % step]

    def run(tag, extra):
        out, edges = tmp_path / ("pose_%s.txt" % tag), tmp_path / ("edges_%s.txt" % tag)
        r = subprocess.run([exe] + common + ["--out", str(out), "--submap-edges", str(edges)] + LOOP_FLAGS + extra, capture_output=True, text=True, timeout=600)
        print(r.stderr[-1500:])
        assert r.returncode == 0, r.returncode
        return out, edges, json.loads(r.stdout.strip().splitlines()[-1])
    corrected = tmp_path / "corrected.txt"
    out0, edges0, line0 = run("plain", [])
    out1, edges1, line1 = run("loops", ["--close-loops", str(corrected)])
    # without the flag: the same files byte for byte, and no new field in the line
    assert out0.read_bytes() == out1.read_bytes() and edges0.read_bytes() == edges1.read_bytes()
    assert not [k for k in line0 if "loop" in k or "pose_graph" in k]
    timing = {"seconds", "pairs_per_s", "submap_seconds", "read_upload_prepare_s_rank0", "wait_for_readers_s_rank0", "upload_s_rank0",
              "prepare_targets_s_rank0", "warmup_batch_before_the_clock_s", "steady_state_pairs_per_s_rank0", "poses_file", "submap_edges_file"}
    assert {k: v for k, v in line0.items() if k not in timing} == {k: v for k, v in line1.items() if k in line0 and k not in timing}
    print({k: v for k, v in line1.items() if k not in line0})
    assert line1["loop_submaps"] == N_SCANS // 3 and line1["pose_graph_solves"] >= N_SCANS // 3 - 1 and line1["pose_graph_stop_reason"] in (1, 2)
    got, raw = kitti.read_poses(str(corrected)), kitti.read_poses(str(out1))
    assert got.shape == raw.shape == (N_SCANS, 4, 4) and np.array_equal(got[0], np.eye(4))
    # scan PERIOD + k was taken where scan k was: the closure error of the revisiting scans, before and after
    truth = [np.linalg.inv(poses[0]) @ P for P in poses]
    def closure(T):
        return max(np.linalg.norm((np.linalg.inv(T[k]) @ T[PERIOD + k])[:3, 3]) for k in range(N_SCANS - PERIOD))
    def to_truth(T):
        return max(np.linalg.norm(T[k][:3, 3] - truth[k][:3, 3]) for k in range(N_SCANS))
    print("closure error: %.4f m as written, %.4f m corrected; worst distance to the truth: %.4f m, %.4f m" % (closure(raw), closure(got), to_truth(raw), to_truth(got)))
    # (Reported, not asserted: on this short, tight circle the driver's own scan-to-scan poses -- a fixed forward guess without
    # rotation at 5.7 degrees a scan -- end tens of metres from the truth, so the detector never sees the revisit and no loop edge
    # is added; the corrected file is then the chain of the submap matches.  That IsamOptimizer::AddFrame closes a loop on the
    # device is test_pose_graph_gpu.py::test_isam_optimizer_pulls_a_drifted_returning_leg_back.)
    print("loop edges:", line1["loop_edges"])
    # inside a submap the frames keep their relative poses (UpdateInnerFramePose: submap pose x local pose)
    for k in range(0, N_SCANS - N_SCANS % 3, 3):
        for f in (1, 2):
            want, have = np.linalg.inv(raw[k]) @ raw[k + f], np.linalg.inv(got[k]) @ got[k + f]
            assert np.abs(want - have).max() < 1e-5                  # (the files carry 8 significant digits)
    # --map-poses takes the corrected file
    pcd = tmp_path / "corrected_map.pcd"
    r = subprocess.run([exe, "--scans", seq, "--map", str(pcd), "--map-poses", str(corrected)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-1500:]
    m = json.loads(r.stdout.strip().splitlines()[-1])
    assert m["map_frames"] == N_SCANS and m["map_points"] > 1000 and pcd.stat().st_size > 1000
