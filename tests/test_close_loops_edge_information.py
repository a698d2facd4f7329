"""smhip_shard --close-loops --edge-information 1 [--edge-information-scale S] [--edge-report FILE]: the consecutive-submap edges (and
the loop edges the detector accepts) are measured with their own 6x6 information and enter the pose graph with it; the report has a
line per such edge.  The refusals run without a GPU.  On the device: a short straight drive, six submaps of two scans; with
--edge-information 0 every output has the bytes of a run without the flag; the report's lines are well formed; the scale reaches
the measurement (the strengths are linear in it)."""
import json
import subprocess

import numpy as np
import pytest

N_SCANS, STEP = 8, 0.5
FLAGS = ["--submap-frames", "2", "--loop-use-descriptor", "0"]


def _exe():
    from staticmapping_amd import build
    build.build()
    return build.build_shard_driver()


def test_the_flags_are_parsed_and_refused_where_they_mean_nothing():
    exe = _exe()

    def err(*flags):
        r = subprocess.run([exe, "--scans", "/nonexistent-dir"] + list(flags), capture_output=True, text=True)
        assert r.returncode == 2
        return r.stderr
    for flags in (("--edge-information", "1"), ("--edge-information-scale", "2"), ("--edge-report", "r.txt")):
        assert "need --close-loops" in err(*flags)
    assert "need --edge-information 1" in err("--close-loops", "x.txt", "--edge-information-scale", "2")
    assert "need --edge-information 1" in err("--close-loops", "x.txt", "--edge-information", "0", "--edge-report", "r.txt")
    for bad in ("0", "-1", "nan", "inf", "1x", ""):
        assert "bad edge setting" in err("--close-loops", "x.txt", "--edge-information", "1", "--edge-information-scale", bad)
    assert "cannot open" in err("--close-loops", "x.txt", "--edge-information", "1", "--edge-information-scale", "0.5", "--edge-report", "r.txt")
    assert "--edge-report FILE" in err("--no-such-flag")                 # the usage text names them


@pytest.fixture(scope="module")
def straight_drive(tmp_path_factory):
    from staticmapping_amd import kitti, synth
    d = tmp_path_factory.mktemp("straight")
    poses = [synth.make_pose(t=(STEP * k, 0.0, 0.0), rpy_deg=(0, 0, 0)) for k in range(N_SCANS)]
    scene = synth.make_drive_scene(poses, seed=11)
    for k, P in enumerate(poses):
        kitti.write_bin(kitti.scan_path(str(d), k), synth.velodyne_scan(synth.scene_near(scene, P[:3, 3]), P, seed=3000 + k, n_points=10_000))
    return str(d)


def _report(path):
    rows = []
    for line in path.read_text().splitlines():
        f = line.split()
        assert len(f) == 17 and f[2] in ("chain", "loop")
        rows.append(dict(i=int(f[0]), j=int(f[1]), kind=f[2], kept=int(f[3]), residual_sigma=float(f[4]),
                         strength=np.array(f[5:11], float), weakest=np.array(f[11:17], float)))
    return rows


@pytest.mark.gpu
def test_the_driver_measures_its_edges_and_reports_them(straight_drive, tmp_path):
    from staticmapping_amd import kitti
    exe = _exe()
    common = [exe, "--scans", straight_drive, "--gpus", "1", "--batch", "8", "--iterations", "30", "--guess-tx", "%.4f" % STEP] + FLAGS

    def run(tag, extra):
        out, corrected = tmp_path / ("pose_%s.txt" % tag), tmp_path / ("corrected_%s.txt" % tag)
        r = subprocess.run(common + ["--out", str(out), "--close-loops", str(corrected)] + extra, capture_output=True, text=True, timeout=300)
        print(r.stderr[-1500:])
        assert r.returncode == 0, r.returncode
        return out, corrected, json.loads(r.stdout.strip().splitlines()[-1])
    out0, cor0, line0 = run("plain", [])
    assert "edge_informations" not in line0
    rep_a, rep_b = tmp_path / "edges_a.txt", tmp_path / "edges_b.txt"
    out2, cor2, line2 = run("on", ["--edge-information", "1", "--edge-report", str(rep_a)])
    out3, cor3, line3 = run("scaled", ["--edge-information", "1", "--edge-information-scale", "0.25", "--edge-report", str(rep_b)])
    assert out2.read_bytes() == out0.read_bytes()                         # the alignment run itself is untouched
    a, b = _report(rep_a), _report(rep_b)
    S = N_SCANS // 2
    print("edges with an information:", line2["edge_informations"], "loop edges:", line2["loop_edges"])
    assert len(a) == line2["edge_informations"] == len(b) == line3["edge_informations"]
    chain = [r for r in a if r["kind"] == "chain"]
    assert 1 <= len(chain) <= S - 1 and len(a) - len(chain) <= line2["loop_edges"]
    assert [r["kind"] for r in a] == sorted((r["kind"] for r in a), key=lambda k: k != "chain")     # chain edges first
    for r, q in zip(a, b):
        print(r["i"], r["j"], r["kind"], "kept", r["kept"], "residual sigma", r["residual_sigma"], "strength", r["strength"], "weakest", r["weakest"])
        assert (r["i"], r["j"], r["kind"], r["kept"]) == (q["i"], q["j"], q["kind"], q["kept"])
        assert r["kind"] == "loop" or r["j"] == r["i"] + 1
        assert r["kept"] > 6 and r["residual_sigma"] >= 0.02 and (r["strength"] >= 0.0).all() and (np.diff(r["strength"]) >= 0.0).all()
        assert abs(np.linalg.norm(r["weakest"]) - 1.0) < 1e-6 and r["weakest"][np.argmax(np.abs(r["weakest"]))] > 0.0
        # the same measurement under another scale: h is linear in it (the file carries 8 significant digits)
        assert np.allclose(q["strength"], 0.25 * r["strength"], rtol=1e-6, atol=0.0) and q["residual_sigma"] == r["residual_sigma"]
    got = kitti.read_poses(str(cor2))
    assert got.shape == (N_SCANS, 4, 4) and np.isfinite(got).all() and np.array_equal(got[0], np.eye(4))
    print("largest distance between the corrected poses with and without the informations: %.4f m" %
          np.abs(got[:, :3, 3] - kitti.read_poses(str(cor0))[:, :3, 3]).max())
