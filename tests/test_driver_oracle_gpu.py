"""The binary: `smhip_shard` on full-size KITTI-format directories, every relative pose of its kitti_pose.txt against the CPU
oracle computed from the files alone (tests/driver_ref.py) -- not against another device run.  One run with the default batch on
33 scans, then the options that change how a sequence is cut into launches (batch size, two matchers, stream parts, readers,
warm-up, early exit) on the first 12 pairs of the full-size and of the ragged directory, each against the same oracle rows; and
what the driver does with a scan that holds no finite point, or no point at all.  Tolerance: BASELINE.json's 1e-4 rad / 1e-3 m;
the file's 8 significant digits cost less than 1 % of it (tests/test_driver_ref.py)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import driver_ref as dr

PRINTED_SCORE_DECIMALS = 0.5e-6            # the line prints mean_score with six decimals


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    return dr.sequence_sets(tmp_path_factory)


@pytest.fixture(scope="module")
def exe():
    from staticmapping_amd import build
    build.build()
    return build.build_shard_driver()


@pytest.fixture(scope="module")
def runs():
    return {}


def _run(exe, scans_dir, out, args, timeout=300):
    """One run of the binary, one subprocess; a non-zero exit ends the test with its stderr."""
    cmd = [exe, "--scans", scans_dir, "--gpus", "1", "--guess-tx", str(dr.GUESS_TX), "--out", str(out)] + list(args)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode < 0 or r.returncode in (134, 139):
        # the driver died on a signal: nothing more is started on a device it may have left in a bad state
        pytest.exit(f"{' '.join(cmd)} died with status {r.returncode}: {r.stderr[-2000:]}", returncode=1)
    assert r.returncode == 0, (" ".join(cmd), r.returncode, r.stderr[-2000:], r.stdout[-500:])
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, open(out).read()


def _variant(runs, exe, sets, tmp_path_factory, which, args):
    key = (which, tuple(args))
    if key not in runs:
        out = tmp_path_factory.mktemp("poses") / "kitti_pose.txt"
        runs[key] = _run(exe, sets[which + "_dir"], out, args) + (str(out),)
    return runs[key]


def _against_the_oracle(o, line, out_path, n_pairs, early_exit=False):
    """Every relative pose of the file and the line's mean score against the oracle's rows; returns the worst figures."""
    assert line["pairs"] == n_pairs and line["unfinished_pairs"] == 0, line
    poses = dr.read_chain(out_path)
    assert poses.shape == (n_pairs + 1, 4, 4) and np.array_equal(poses[0], np.eye(4))
    rel = dr.relative_poses(poses)
    worst = [0.0, 0.0]
    ref = [o.pair(k, early_exit=early_exit) for k in range(n_pairs)]
    for k in range(n_pairs):
        da, dt = dr.se3_error(rel[k], ref[k]["result"])
        print(f"pair {k}: {da:.2e} rad {dt:.2e} m")
        assert da < dr.ROT_TOL and dt < dr.TRANS_TOL, (k, da, dt)
        worst = [max(worst[0], da), max(worst[1], dt)]
    mean_score = float(np.mean([r["score"] for r in ref]))
    ds = abs(line["mean_score"] - mean_score)
    assert ds < dr.SCORE_TOL + PRINTED_SCORE_DECIMALS, (line["mean_score"], mean_score)
    return worst + [ds], float(np.mean([r["iterations"] for r in ref]))


@pytest.mark.gpu
def test_default_batch_on_33_full_size_scans(sets, exe, runs, tmp_path_factory, capsys):
    line, _, out = _variant(runs, exe, sets, tmp_path_factory, "full", ["--iterations", "20"])
    assert line["batch"] == 32 and line["mean_iterations"] == 20, line
    worst, _ = _against_the_oracle(sets["full"], line, out, 32)
    with capsys.disabled():
        print(f"\n[smhip_shard vs oracle, 33 full-size scans, one batch of 32] worst {worst[0]:.2e} rad / {worst[1]:.2e} m, mean score {worst[2]:.1e}")


MATRIX = [
    ("full", ["--batch", "1"]),                          # twelve single-pair batches: the one launch, the target replaced every time
    ("full", ["--batch", "5"]),                          # 5, 5, 2: a grid row per pair, a shorter tail
    ("ragged", ["--batch", "5"]),
    ("full", ["--batch", "12"]),                         # between the forms
    ("ragged", ["--batch", "12"]),
    ("full", ["--batch", "7"]),                          # 7, 5
    ("full", ["--batch", "5", "--matchers", "2"]),       # two handles take turns (12 pairs > 5)
    ("ragged", ["--batch", "5", "--matchers", "2"]),
    ("full", ["--batch", "12", "--parts", "1"]),         # stream parts
    ("full", ["--batch", "12", "--parts", "3"]),
    ("full", ["--batch", "12", "--readers", "1"]),       # a single reader
]


@pytest.mark.gpu
@pytest.mark.parametrize("which,args", MATRIX, ids=[w + ":" + " ".join(a) for w, a in MATRIX])
def test_option_matrix_against_the_oracle(sets, exe, runs, tmp_path_factory, which, args, capsys):
    full_args = ["--max-pairs", "12", "--iterations", "20"] + args
    line, _, out = _variant(runs, exe, sets, tmp_path_factory, which, full_args)
    assert line["batch"] == int(args[1]) and line["mean_iterations"] == 20, line
    worst, _ = _against_the_oracle(sets[which], line, out, 12)
    with capsys.disabled():
        print(f"\n[smhip_shard vs oracle, {which}, {' '.join(args)}] 12 pairs: worst {worst[0]:.2e} rad / {worst[1]:.2e} m, mean score {worst[2]:.1e}")


@pytest.mark.gpu
def test_without_the_warm_up_batch_the_file_is_the_same_bytes(sets, exe, runs, tmp_path_factory):
    base = ["--max-pairs", "12", "--iterations", "20", "--batch", "12"]
    line, text, _ = _variant(runs, exe, sets, tmp_path_factory, "full", base)
    line0, text0, out0 = _variant(runs, exe, sets, tmp_path_factory, "full", base + ["--warmup", "0"])
    assert line["warmup_batch_before_the_clock_s"] > 0 and line0["warmup_batch_before_the_clock_s"] == 0
    assert text0 == text
    _against_the_oracle(sets["full"], line0, out0, 12)


@pytest.mark.gpu
def test_early_exit_run_against_the_early_exit_oracle(sets, exe, runs, tmp_path_factory, capsys):
    """The same tolerance holds with the early exit on: the oracle moves by less than half of it when it stops one iteration
    sooner or later (tests/test_driver_ref.py), so a device that stops one iteration off on its own target still has to pass."""
    args = ["--max-pairs", "12", "--batch", "12", "--early-exit", "1", "--iterations", "100"]
    line, _, out = _variant(runs, exe, sets, tmp_path_factory, "full", args)
    worst, oracle_mean_it = _against_the_oracle(sets["full"], line, out, 12, early_exit=True)
    with capsys.disabled():
        print(f"\n[smhip_shard vs oracle, full, early exit] 12 pairs: worst {worst[0]:.2e} rad / {worst[1]:.2e} m, mean score {worst[2]:.1e}; "
              f"mean iterations {line['mean_iterations']} (oracle {oracle_mean_it:.2f})")
    assert line["mean_iterations"] < 25                                       # far below the 100 allowed
    assert abs(line["mean_iterations"] - oracle_mean_it) <= 1.0 + 0.005       # no pair more than one iteration off; two printed decimals


def _copy_with(src_dir, dst_dir, index, content):
    os.makedirs(dst_dir)
    for f in sorted(os.listdir(src_dir)):
        shutil.copy(os.path.join(src_dir, f), os.path.join(dst_dir, f))
    victim = os.path.join(dst_dir, sorted(os.listdir(dst_dir))[index])
    with open(victim, "wb") as f:
        f.write(content)
    return victim


@pytest.mark.gpu
def test_a_scan_without_a_finite_point_ends_the_run_by_name(sets, exe, tmp_path):
    """The ragged directory with scan 6 replaced by an all-NaN file of the same size.  The driver's contract is the loud one: it
    ends non-zero naming the file before that scan reaches the device, and writes no pose file -- never exit 0 with a chained pose
    for pairs 5 and 6."""
    size = dr.RAGGED_SIZES[6]
    victim = _copy_with(sets["ragged_dir"], str(tmp_path / "seq"), 6, np.full((size, 4), np.nan, dtype=np.float32).tobytes())
    assert os.path.getsize(victim) == 16 * size
    out = tmp_path / "kitti_pose.txt"
    r = subprocess.run([exe, "--scans", str(tmp_path / "seq"), "--gpus", "1", "--guess-tx", str(dr.GUESS_TX), "--out", str(out), "--iterations", "20"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "holds no finite point" in r.stderr and os.path.basename(victim) in r.stderr, r.stderr[-2000:]
    # no pose file and no result line (the collective library prints its version banner to stdout when it starts)
    assert not out.exists()
    assert not any(ln.lstrip().startswith("{") for ln in r.stdout.splitlines()), r.stdout[-500:]


def test_an_empty_file_ends_the_run_by_name_before_any_device_work(exe, tmp_path):
    """A 0-byte scan in the sequence: smhip_set_sources_f32_batch refuses n <= 0 without knowing the file, so the driver checks
    the files first and names the one.  No GPU is needed to get there."""
    from staticmapping_amd import kitti
    d = tmp_path / "seq"
    d.mkdir()
    rng = np.random.default_rng(0)
    for k in range(3):
        kitti.write_bin(kitti.scan_path(str(d), k), rng.normal(size=(100, 4)).astype(np.float32))
    victim = kitti.scan_path(str(d), 1)
    open(victim, "wb").close()
    out = tmp_path / "kitti_pose.txt"
    r = subprocess.run([exe, "--scans", str(d), "--gpus", "1", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "holds no point" in r.stderr and os.path.basename(victim) in r.stderr, r.stderr[-2000:]
    assert not out.exists()
