"""smhip_shard --close-loops --pose-covariance: runs on the 72-scan circle drive of test_close_loops_gpu.py (once round a circle and on
over its first nine scans), submaps of three scans; after the final optimisation the driver writes every submap's marginal covariance
(include/smhip.h, "Marginal covariances"), one line per submap: index held sigma_rot[3] sigma_pos_world[3] cov[21].  What the file
holds is checked against a replay: --pose-graph-dump writes the final optimisation's input, the test runs the same solve on a handle of
its own (the same entry's bits: every optimise entry gives the bits of the one below it when the extra arrays name nothing) and asks
pose_graph.marginals for the same nodes at that handle state."""
import json
import subprocess

import numpy as np
import pytest

from test_close_loops_gpu import LOOP_FLAGS, N_SCANS, PERIOD, RADIUS, circle_drive  # noqa: F401  (the fixture)


def test_the_flag_needs_close_loops_and_a_path_it_can_write(tmp_path):
    from staticmapping_amd import build
    build.build()
    exe = build.build_shard_driver()
    cov = tmp_path / "cov.txt"
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--pose-covariance", str(cov)], capture_output=True, text=True)
    assert r.returncode == 2 and "--pose-covariance needs --close-loops" in r.stderr
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", str(tmp_path / "x.txt"), "--pose-graph-dump", str(tmp_path / "g.txt")], capture_output=True, text=True)
    assert r.returncode == 2 and "need --pose-covariance" in r.stderr
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", str(tmp_path / "x.txt"), "--pose-covariance", str(cov), "--pose-covariance-chunk", "0"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "at least 1" in r.stderr
    # the flag is known: the run gets as far as the scans -- and neither creates the file nor touches one that is there
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", str(tmp_path / "x.txt"), "--pose-covariance", str(cov)], capture_output=True, text=True)
    assert r.returncode == 2 and "cannot open" in r.stderr and not cov.exists()
    cov.write_text("kept\n")
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", str(tmp_path / "x.txt"), "--pose-covariance", str(cov)], capture_output=True, text=True)
    assert r.returncode == 2 and cov.read_text() == "kept\n"
    bad = tmp_path / "no-such-dir" / "cov.txt"
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", str(tmp_path / "x.txt"), "--pose-covariance", str(bad)], capture_output=True, text=True)
    assert r.returncode == 2 and "cannot write" in r.stderr and str(bad) in r.stderr      # a bad path: before any work
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", str(tmp_path / "x.txt"), "--pose-covariance", str(cov), "--pose-graph-dump", str(bad)],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "cannot write" in r.stderr and str(bad) in r.stderr


def _upper(c21):
    C = np.zeros((6, 6))
    C[np.triu_indices(6)] = c21
    return C + np.triu(C, 1).T


def _read_dump(path):
    """the driver's --pose-graph-dump: dict(poses [n, 4, 4], fixed [n], kinds [m], ij [m, 2], data [m, 16], sigmas [m, 6], huber [m], L [m] of None or [6, 6])"""
    lines = path.read_text().splitlines()
    n, m = (int(v) for v in lines[0].split())
    assert len(lines) == 1 + n + m
    nodes = np.array([[float(v) for v in ln.split()] for ln in lines[1:1 + n]])
    g = dict(poses=nodes[:, :16].reshape(n, 4, 4).transpose(0, 2, 1), fixed=nodes[:, 16].astype(np.uint8), kinds=[], ij=[], data=[], sigmas=[], huber=[], L=[])
    for ln in lines[1 + n:]:
        v = ln.split()
        g["kinds"].append(int(v[0])); g["ij"].append((int(v[1]), int(v[2])))
        g["data"].append([float(x) for x in v[3:19]]); g["sigmas"].append([float(x) for x in v[19:25]]); g["huber"].append(float(v[25]))
        g["L"].append(np.array([float(x) for x in v[27:63]]).reshape(6, 6) if int(v[26]) else None)
        assert len(v) == 27 + (36 if int(v[26]) else 0)
    for key in ("kinds", "ij", "data", "sigmas", "huber"):
        g[key] = np.array(g[key])
    return g


def _replay(handle, g, nodes):
    """the dumped solve again, then the marginal covariances of `nodes` at that state: (poses, cov)"""
    from staticmapping_amd import pose_graph
    poses, stats = pose_graph.optimize_info(handle, g["poses"], g["kinds"].astype(np.uint8), g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"],
                                            huber=g["huber"] if (g["huber"] != 0.0).any() else None,
                                            sqrt_information=g["L"] if any(L is not None for L in g["L"]) else None)
    assert stats["stop"] in ("step", "cost")
    cov, _, _ = pose_graph.marginals(handle, len(poses), nodes)
    return poses, cov


def _check_lines(rows, poses, cov):
    """every number of every line against the replay, to the file's nine digits"""
    for row, X, C in zip(rows, poses, cov):
        val = np.array([float(v) for v in row[2:]])
        assert len(val) == 6 + 21
        assert np.allclose(val[6:], C[np.triu_indices(6)], rtol=1e-8, atol=0.0)
        assert np.allclose(val[:3], np.sqrt(np.diag(C)[:3]), rtol=1e-8, atol=0.0)
        assert np.allclose(val[3:6], np.sqrt(np.diag(X[:3, :3] @ C[3:, 3:] @ X[:3, :3].T)), rtol=1e-8, atol=0.0)


@pytest.fixture(scope="module")
def handle():
    from staticmapping_amd import IcpFastHip
    m = IcpFastHip(device=0, max_source_points=1024, max_target_points=1024)
    yield m
    m.close()


def _common(exe, seq, tmp_path):
    step = 2.0 * np.pi * RADIUS / PERIOD
    return [exe, "--scans", seq, "--gpus", "1", "--batch", "8", "--iterations", "30", "--guess-tx", "%.4f" % step, "--guess", "ctrv", "--out", str(tmp_path / "pose.txt")] + LOOP_FLAGS


@pytest.mark.gpu
def test_pose_covariance_lines_of_the_circle_drive(circle_drive, handle, tmp_path):  # noqa: F811
    """One line per submap; the held submap all zeros; every other matrix positive definite; the largest position sigma strictly inside
    the ring and not at its end (the loop edges pin the end); and every number of the file -- cov[21], sigma_rot, sigma_pos_world --
    equals, to the file's nine digits, what pose_graph.marginals gives after the dumped final solve is run again.  The driver asks
    ten nodes a call here, so the 24 submaps take three calls."""
    from staticmapping_amd import build, kitti
    seq, _ = circle_drive
    exe = build.build_shard_driver()
    corrected, cov_file, dump = tmp_path / "corrected.txt", tmp_path / "cov.txt", tmp_path / "graph.txt"
    r = subprocess.run(_common(exe, seq, tmp_path) + ["--close-loops", str(corrected), "--pose-covariance", str(cov_file), "--pose-covariance-chunk", "10",
                                                     "--pose-graph-dump", str(dump)], capture_output=True, text=True, timeout=600)
    print(r.stderr[-1500:])
    assert r.returncode == 0, r.returncode
    line = json.loads(r.stdout.strip().splitlines()[-1])
    S = N_SCANS // 3
    print({k: line[k] for k in ("loop_submaps", "loop_edges", "pose_graph_solves", "pose_graph_stop_reason", "pose_covariance_file")})
    assert line["loop_submaps"] == S and line["pose_covariance_file"] == str(cov_file) and "odom_tf_sigmas" not in line
    rows = [ln.split() for ln in cov_file.read_text().splitlines()]
    assert len(rows) == S and [r[0] for r in rows] == [str(k) for k in range(S)] and all(len(r) == 2 + 6 + 21 for r in rows)
    held = np.array([int(r[1]) for r in rows])
    val = np.array([[float(v) for v in r[2:]] for r in rows])
    assert held.tolist() == [1] + [0] * (S - 1) and (val[0] == 0.0).all()
    for k in range(1, S):
        assert (np.linalg.eigvalsh(_upper(val[k, 6:])) > 0.0).all(), k
    sigma = np.linalg.norm(val[:, 3:6], axis=1)
    print("position sigma per submap [m]:", np.round(sigma, 4), "loop edges", line["loop_edges"])
    assert line["loop_edges"] >= 1
    assert 0 < int(np.argmax(sigma)) < S - 1
    # the replay
    g = _read_dump(dump)
    assert len(g["poses"]) == S and len(g["kinds"]) == S - 1 + line["loop_edges"] and g["fixed"].tolist() == held.tolist()
    poses, cov = _replay(handle, g, list(range(S)))
    written = kitti.read_poses(str(corrected))[::3][:S]
    assert np.abs(poses - written).max() < 1e-6                          # the same solve: the corrected poses (eight digits in that file)
    _check_lines(rows, poses, cov)


@pytest.mark.gpu
def test_the_calibration_vertex_has_its_line_and_its_sigmas(circle_drive, handle, tmp_path):  # noqa: F811
    """With --odom --odom-calib the graph has the calibration vertex: the file ends with a line labelled `calib`, the line on stdout
    carries odom_tf_sigmas, and both are the replay's covariance of that node.  Without --pose-covariance the sigmas are there all
    the same."""
    from staticmapping_amd import build
    seq, truth = circle_drive
    exe = build.build_shard_driver()
    odom = tmp_path / "odom.txt"
    first = np.linalg.inv(truth[0])
    odom.write_text("".join(" ".join("%.12g" % v for v in (first @ P)[:3].ravel()) + "\n" for P in truth))
    corrected, cov_file, dump = tmp_path / "corrected.txt", tmp_path / "cov.txt", tmp_path / "graph.txt"
    flags = _common(exe, seq, tmp_path) + ["--close-loops", str(corrected), "--odom", str(odom), "--odom-calib"]
    r = subprocess.run(flags + ["--pose-covariance", str(cov_file), "--pose-graph-dump", str(dump)], capture_output=True, text=True, timeout=600)
    print(r.stderr[-1500:])
    assert r.returncode == 0, r.returncode
    line = json.loads(r.stdout.strip().splitlines()[-1])
    S = N_SCANS // 3
    rows = [ln.split() for ln in cov_file.read_text().splitlines()]
    assert [r[0] for r in rows] == [str(k) for k in range(S)] + ["calib"] and [int(r[1]) for r in rows] == [1] + [0] * S
    g = _read_dump(dump)
    assert len(g["poses"]) == S + 1 and int((g["kinds"] == 3).sum()) == line["odom_factors"] > 0
    poses, cov = _replay(handle, g, list(range(S + 1)))
    _check_lines(rows, poses, cov)
    print("odom_tf_sigmas", line["odom_tf_sigmas"])
    assert np.allclose(line["odom_tf_sigmas"], np.sqrt(np.diag(cov[S])), rtol=1e-8, atol=0.0) and min(line["odom_tf_sigmas"]) > 0.0
    r = subprocess.run(flags, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.returncode
    assert json.loads(r.stdout.strip().splitlines()[-1])["odom_tf_sigmas"] == line["odom_tf_sigmas"]
