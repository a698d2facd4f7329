"""Joining two maps on the device (include/smhip/multi_trajectory.h) through tests/cpp/test_multi_trajectory.cc: hand-fed joins solved by
MultiTrajectoryOptimizer against tests/multi_trajectory_ref.py, a loaded base map solved alone, and MultiTrajectoryMapBuilder end to end
on two generated maps -- descriptors, the loop detector restricted to the base map, the cross-trajectory matches, the one solve, the
joined map and its two PCD outputs."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import multi_trajectory_ref as mt
import test_multi_trajectory_cpp as cpp

pytestmark = pytest.mark.gpu

# Result parity of the hand-fed joins, in metres and in rotation-matrix entries: the comparison and bound of
# tests/test_pose_graph_robust_gpu.py, 1e-9 m / 1e-9 against the restatement's direct solve.  Measured on the MI355X: see
# test_join_graph_matches_the_restatement's docstring.
BOUND = 1e-9


@pytest.mark.parametrize("hold_base", [False, True], ids=["base_free", "base_held"])
@pytest.mark.parametrize("name", list(mt.PARITY))
def test_join_graph_matches_the_restatement(name, hold_base, tmp_path):
    """8 + 8 and 63 + 2, 64 + 1, 1 + 64 (65 nodes: the cyclic reduction gains a level, the joint between the trajectories at either end),
    each with the base free and held, solved through MultiTrajectoryOptimizer on the device from hand-fed cross edges: poses within 1e-9 m
    / 1e-9 of the restatement, the same stop reason and step counts, held base poses bit-equal and one CG iteration per step when held.
    Measured on the MI355X (translation m / rotation entry), base free, then held:
      join8_8   2.9e-14 / 1.1e-15,  3.6e-15 / 3.3e-16        join63_2  2.8e-14 / 1.0e-15,  5.6e-17 / 4.4e-16
      join64_1  1.4e-11 / 7.4e-14,  5.6e-17 / 3.3e-16        join1_64  4.3e-10 / 2.2e-12,  2.8e-14 / 2.0e-15
    join1_64 with the base free is the largest: 61 cross edges leave one free base node, and the restatement's own direct and PCG solves
    of that graph differ by 4.3e-10 m; the device's PCG solve ends where the restatement's does."""
    got = cpp.run_join("gpu", tmp_path, mt.parity_case(name), hold_base)
    dt, dr = cpp.check_join(name, hold_base, got)
    assert dt < BOUND and dr < BOUND


# ---- two generated maps ---------------------------------------------------------------------------------------------------------

DRIFT_T, DRIFT_YAW_DEG = (0.3, 0.4, 0.0), 0.5            # test_pose_graph_gpu.py's drift: 0.5 m, 0.5 degrees
FRAMES, SUBMAPS = 3, 6


def transform_to_vector6(X):
    """common/math.h:153-160 (RotationMatrixToEulerAngles, :108-127)"""
    R = X[:3, :3]
    sy = np.hypot(R[0, 0], R[1, 0])
    assert sy >= 1e-6
    return [X[0, 3], X[1, 3], X[2, 3], np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], sy), np.arctan2(R[1, 0], R[0, 0])]


def write_map(directory, poses, clouds, premultiply=None):
    """directory/map.xml in the reference's format -- one trajectory, each submap connected to the next -- and a cloud file per submap"""
    os.makedirs(directory, exist_ok=True)
    rows = []
    for k, (P, cloud) in enumerate(zip(poses, clouds)):
        with open(os.path.join(directory, "submap_%d.bin" % k), "wb") as fh:
            fh.write(struct.pack("<IIIQ", 0, 0, 1, len(cloud)) + np.ascontiguousarray(cloud, "<f4").tobytes())
        v = transform_to_vector6(P if premultiply is None else premultiply @ P)
        rows.append('\t\t<Submap id="%d" file="submap_%d.bin" tx="%.17g" ty="%.17g" tz="%.17g" rx="%.17g" ry="%.17g" rz="%.17g" connections="%s" />\n'
                    % ((k, k) + tuple(v) + ("[0,%d]" % (k + 1) if k + 1 < len(poses) else "",)))
    with open(os.path.join(directory, "map.xml"), "w") as fh:
        fh.write('<?xml version="1.0"?>\n<Map>\n\t<Trajectory id="0" enu_x="0" enu_y="0">\n' + "".join(rows) + "\t</Trajectory>\n</Map>\n")
    return os.path.join(directory, "map.xml")


@pytest.fixture(scope="module")
def two_maps(tmp_path_factory):
    """The scene and sizes of test_pose_graph_gpu.py::test_isam_optimizer_pulls_a_drifted_returning_leg_back: 20 000-point scans, submaps of
    three.  Six submaps along a path are the base map; a second pass over the same poses with other scan seeds is the incremental map,
    its map.xml poses premultiplied by the drift."""
    from staticmapping_amd import synth
    d = tmp_path_factory.mktemp("join")
    truth = [synth.make_pose(t=(0.8 * k, 0.03 * k, 0.0), rpy_deg=(0, 0, 0.6 * k)) for k in range(FRAMES * SUBMAPS)]
    scene = synth.make_scene(0)

    def submaps(seed0):
        out = []
        for s in range(SUBMAPS):
            rows = []
            for f in range(FRAMES):
                k = FRAMES * s + f
                scan = synth.velodyne_scan(scene, truth[k], seed=seed0 + k, n_points=20_000)
                local = (np.linalg.inv(truth[FRAMES * s]) @ truth[k]).astype(np.float32)          # Submap::InsertFrame: into the first frame's coordinates
                xyz = scan[:, :3] @ local[:3, :3].T + local[:3, 3]
                rows.append(np.concatenate([xyz, scan[:, 3:4], np.linspace(0, 1, len(scan), endpoint=False, dtype=np.float32)[:, None]], axis=1))
            out.append(np.concatenate(rows).astype(np.float32))
        return out
    first = [truth[FRAMES * s] for s in range(SUBMAPS)]
    drift = synth.make_pose(t=DRIFT_T, rpy_deg=(0, 0, DRIFT_YAW_DEG))
    base = write_map(str(d / "base"), first, submaps(300))
    inc = write_map(str(d / "inc"), first, submaps(700), premultiply=drift)
    return dict(dir=d, base=base, inc=inc, truth=np.stack(first), loaded=np.stack([drift @ P for P in first]))


def _run(args, timeout=300):
    out = subprocess.run([cpp._build_exe()] + [str(a) for a in args], text=True, capture_output=True, timeout=timeout)
    print(out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_loaded_base_map_is_at_its_optimum(two_maps):
    """after LoadBaseMap every factor's residual is exactly zero: a forced solve starts at cost 0.0 and leaves every pose's bits"""
    res = _run(["base", "gpu", two_maps["base"]])
    print(res)
    assert res["ok"] and res["submaps"] == SUBMAPS and res["factors"] == SUBMAPS and res["solves"] == 1
    assert res["initial_cost"] == 0.0
    assert res["a_bit_moved"] is False


def _inv(X):
    Y = np.eye(4)
    Y[:3, :3] = X[:3, :3].T
    Y[:3, 3] = -X[:3, :3].T @ X[:3, 3]
    return Y


@pytest.mark.parametrize("hold_base", [0, 1], ids=["base_free", "base_held"])
def test_join_pulls_a_shifted_second_drive_onto_the_base(two_maps, hold_base):
    """At every incremental submap that received a loop edge the error of base_k^-1 incremental_k against the truth (the identity: the
    second pass stood where the first did) is below 0.5 of what it was as loaded -- test_pose_graph_gpu.py's own condition; with the base
    held the same holds against the absolute truth."""
    d = two_maps["dir"]
    out = d / ("joined_%d.xml" % hold_base)
    args = ["join", "gpu", two_maps["base"], two_maps["inc"], out, hold_base, "0.98"]
    if hold_base:
        args += [d / "whole.pcd", d / "static.pcd"]
    res = _run(args)
    print({k: v for k, v in res.items() if k != "trajectories"})
    assert res["ok"] and res["base_submaps"] == SUBMAPS and res["incremental_submaps"] == SUBMAPS and res["solves"] == 1
    assert res["loop_edges"] >= 2 and len(res["edges"]) == res["loop_edges"]
    assert all(tt == 0 and st == 1 for tt, _, st, _, _, _ in res["edges"])                  # every edge joins two different trajectories
    assert all(ts < SUBMAPS - 1 for _, ts, _, _, _, _ in res["edges"])                      # the last base submap is never a candidate
    assert res["stop_reason"] in (1, 2)
    assert res["clouds_in_memory"] <= 4 and res["cloud_loads"] > 4                          # the clouds were not all held at once
    base = np.array([s["pose"] for s in res["trajectories"][0]]).reshape(SUBMAPS, 4, 4)
    inc = np.array([s["pose"] for s in res["trajectories"][1]]).reshape(SUBMAPS, 4, 4)
    truth, loaded = two_maps["truth"], two_maps["loaded"]
    with_edge = sorted({ss for _, _, _, ss, _, _ in res["edges"]})
    for s in with_edge:
        before = np.linalg.norm((_inv(truth[s]) @ loaded[s])[:3, 3])
        after = np.linalg.norm((_inv(base[s]) @ inc[s])[:3, 3])
        print("submap %d: mutual error %.3f m as loaded, %.3f m after, factor %.3f" % (s, before, after, after / before))
        assert before > 0.45 and after < 0.5 * before
        if hold_base:
            before_abs, after_abs = np.linalg.norm(loaded[s][:3, 3] - truth[s][:3, 3]), np.linalg.norm(inc[s][:3, 3] - truth[s][:3, 3])
            print("          absolute %.3f m as loaded, %.3f m after" % (before_abs, after_abs))
            assert after_abs < 0.5 * before_abs
    # the connection lists: the base submaps that were matched name their sources in trajectory 1, the incremental map's own are offset
    for tt, ts, st, ss, _, _ in res["edges"]:
        assert "[%d,%d]" % (st, ss) in res["trajectories"][0][ts]["connections"]
    assert [s["connections"] for s in res["trajectories"][1]] == ["[1,%d]" % (k + 1) if k + 1 < SUBMAPS else "" for k in range(SUBMAPS)]
    if hold_base:
        # the base map as read: Vector6ToTransform of the six numbers written above, to the last bit through %.17g
        assert res["pcg_max_iterations"] == 1
        assert np.abs(base - truth).max() < 1e-12
        assert res["whole_map_points"] == 2 * SUBMAPS * FRAMES * 20_000 and res["static_map_voxels"] > 1000
        for name in ("whole.pcd", "static.pcd"):
            head = open(d / name, "rb").read(400).decode("ascii", "replace")
            points = int(head.split("POINTS ")[1].split("\n")[0])
            assert points > 1000 and "DATA binary\n" in head
    else:
        assert np.abs(base - truth).max() > 1e-6                                            # free: the base map moves as well
    text = open(out).read()
    assert text.count("<Trajectory ") == 2 and 'id="1"' in text and text.count("<Submap ") == 2 * SUBMAPS
