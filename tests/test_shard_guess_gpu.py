"""smhip_shard --guess constant|ctrv.  With ctrv the driver aligns the pairs of a batch one after the other, pair k + 1 from
front_end::CtrvGuessFromLast of pair k's result, the first pair of a batch from the last result of the batch before it.

Fixture: the circle of tests/test_close_loops_gpu.py (72 scans once round 12 m and on over the first nine, 5.7 degrees a scan, the same
seeds) at 20 000 points a scan.  On the CPU the oracle's chain closes this circle to 0.44 m; the constant guess leaves tens of metres."""
import json
import subprocess

import numpy as np
import pytest

import driver_ref as dr

N_SCANS, PERIOD, RADIUS = 72, 63, 12.0
N_POINTS = 20_000
STEP = 2.0 * np.pi * RADIUS / PERIOD
LOOP_FLAGS = ["--submap-frames", "3", "--loop-ignore-threshold", "6", "--loop-max-distance", "5", "--loop-use-descriptor", "0"]    # test_close_loops_gpu.py's
LOOP_MAX_DISTANCE = 5.0


@pytest.fixture(scope="module")
def exe():
    from staticmapping_amd import build
    build.build()
    return build.build_shard_driver()


def test_guess_flag_refusals(exe):
    def run(*flags):
        return subprocess.run([exe, "--scans", "/nonexistent-dir"] + list(flags), capture_output=True, text=True, timeout=60)
    r = run("--guess", "ctrv", "--gpus", "2")
    assert r.returncode == 2 and "--guess ctrv" in r.stderr and "--gpus" in r.stderr, r.stderr
    r = run("--guess", "ctrv", "--matchers", "2")
    assert r.returncode == 2 and "--guess ctrv" in r.stderr and "--matchers" in r.stderr, r.stderr
    r = run("--guess", "sideways")
    assert r.returncode == 2 and "--guess" in r.stderr and "sideways" in r.stderr, r.stderr
    for value in ("ctrv", "constant"):                     # known values get as far as the scans
        r = run("--guess", value)
        assert r.returncode == 2 and "cannot open" in r.stderr, r.stderr


@pytest.fixture(scope="module")
def circle(tmp_path_factory):
    from staticmapping_amd import kitti, synth
    d = tmp_path_factory.mktemp("circle20k")
    poses = []
    for k in range(N_SCANS):
        a = 2.0 * np.pi * k / PERIOD
        poses.append(synth.make_pose(t=(RADIUS * np.sin(a), RADIUS * (1.0 - np.cos(a)), 0.0), rpy_deg=(0, 0, np.rad2deg(a))))
    scene = synth.make_drive_scene(poses, seed=7)
    for k, P in enumerate(poses):
        kitti.write_bin(kitti.scan_path(str(d), k), synth.velodyne_scan(synth.scene_near(scene, P[:3, 3]), P, seed=2000 + k, n_points=N_POINTS))
    return str(d), poses


@pytest.fixture(scope="module")
def runs(exe, circle, tmp_path_factory):
    """one run of the binary per set of flags, shared by the tests below"""
    seq, _ = circle
    root = tmp_path_factory.mktemp("guess_runs")
    done = {}

    def run(tag, flags):
        if tag not in done:
            out = root / ("pose_%s.txt" % tag)
            cmd = [exe, "--scans", seq, "--gpus", "1", "--iterations", "30", "--guess-tx", "%.4f" % STEP, "--out", str(out)] + list(flags)
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode < 0 or r.returncode in (134, 139):
                pytest.exit(f"{' '.join(cmd)} died with status {r.returncode}: {r.stderr[-2000:]}", returncode=1)
            assert r.returncode == 0, (" ".join(cmd), r.returncode, r.stderr[-2000:], r.stdout[-500:])
            done[tag] = (json.loads(r.stdout.strip().splitlines()[-1]), dr.read_chain(str(out)), root)
        return done[tag]
    return run


def _closure(T):
    """scan PERIOD + k was taken where scan k was"""
    return max(np.linalg.norm((np.linalg.inv(T[k]) @ T[PERIOD + k])[:3, 3]) for k in range(N_SCANS - PERIOD))


def _to_truth(T, poses):
    truth = [np.linalg.inv(poses[0]) @ P for P in poses]
    return max(np.linalg.norm(T[k][:3, 3] - truth[k][:3, 3]) for k in range(N_SCANS))


@pytest.mark.gpu
def test_ctrv_poses_close_the_circle(runs, circle, capsys):
    _, poses = circle
    line, T, _ = runs("ctrv8", ["--guess", "ctrv", "--batch", "8"])
    assert line["guess"] == "ctrv" and line["pairs"] == N_SCANS - 1 and line["batch"] == 8, line
    assert line["unfinished_pairs"] == 0, line
    assert T.shape == (N_SCANS, 4, 4)
    c_ctrv = _closure(T)
    line0, T0, _ = runs("constant8", ["--guess", "constant", "--batch", "8"])
    assert "guess" not in line0                                   # the default's line is what it was
    c_const = _closure(T0)
    with capsys.disabled():
        print(f"\n[smhip_shard --guess, circle at {N_POINTS} points] closure: ctrv {c_ctrv:.3f} m (worst distance to the truth {_to_truth(T, poses):.3f} m, "
              f"mean iterations {line['mean_iterations']}), constant {c_const:.3f} m ({_to_truth(T0, poses):.3f} m)")
    assert c_ctrv < LOOP_MAX_DISTANCE, c_ctrv                     # the condition under which the detector can see a revisit at all
    assert c_ctrv < c_const, (c_ctrv, c_const)


@pytest.mark.gpu
def test_the_default_is_the_constant_guess(runs):
    line0, T0, _ = runs("constant8", ["--guess", "constant", "--batch", "8"])
    line1, T1, _ = runs("default8", ["--batch", "8"])
    assert np.array_equal(T0, T1) and "guess" not in line1


@pytest.mark.gpu
def test_a_batch_boundary_does_not_show(runs, capsys):
    """--batch 8 cuts the 71 pairs into nine batches (eight boundaries: the guess is carried across them); --batch 71 is one batch.
    Every pair's relative pose agrees within what the two files' 8 significant digits can move
    it plus the project's tolerance for two runs of one Align."""
    _, Ta, _ = runs("ctrv8", ["--guess", "ctrv", "--batch", "8"])
    line, Tb, _ = runs("ctrv71", ["--guess", "ctrv", "--batch", "71"])
    assert line["batch"] == N_SCANS - 1 and line["unfinished_pairs"] == 0, line
    ra, rb = dr.relative_poses(Ta), dr.relative_poses(Tb)
    fa, fb = dr.file_precision_bound(Ta), dr.file_precision_bound(Tb)
    worst = [0.0, 0.0]
    for k in range(N_SCANS - 1):
        da, dt = dr.se3_error(ra[k], rb[k])
        worst = [max(worst[0], da), max(worst[1], dt)]
        assert da < fa[0] + fb[0] + dr.ROT_TOL and dt < fa[1] + fb[1] + dr.TRANS_TOL, (k, da, dt)
    with capsys.disabled():
        print(f"\n[--batch 8 vs --batch 71, ctrv] worst relative-pose difference {worst[0]:.2e} rad / {worst[1]:.2e} m "
              f"(file precision {fa[0] + fb[0]:.1e} rad / {fa[1] + fb[1]:.1e} m)")


@pytest.mark.gpu
def test_close_loops_on_ctrv_poses(runs, circle, capsys):
    from staticmapping_amd import kitti
    _, poses = circle
    _, _, root = runs("ctrv8", ["--guess", "ctrv", "--batch", "8"])
    corrected = root / "corrected_ctrv.txt"
    line, raw, _ = runs("ctrv8_loops", ["--guess", "ctrv", "--batch", "8", "--close-loops", str(corrected)] + LOOP_FLAGS)
    got = kitti.read_poses(str(corrected))
    assert got.shape == raw.shape == (N_SCANS, 4, 4)
    assert line["loop_submaps"] == N_SCANS // 3, line
    with capsys.disabled():
        print(f"\n[--guess ctrv --close-loops] loop edges {line['loop_edges']}; closure {_closure(raw):.3f} m as written, {_closure(got):.3f} m corrected; "
              f"worst distance to the truth {_to_truth(raw, poses):.3f} m, {_to_truth(got, poses):.3f} m; "
              + ", ".join(f"{k}: {v}" for k, v in line.items() if "loop" in k or "pose_graph" in k))
    # (the first run on an MI355X: 8 loop edges, closure 0.444 m as written and 0.014 m corrected, 0.473 m / 0.054 m to the truth)
    assert line["loop_edges"] >= 1, line
    assert _closure(got) < _closure(raw), (_closure(got), _closure(raw))
