"""smhip_shard --close-loops --loop-guess-search 1 [--loop-guess-resolution R] [--loop-guess-window half_xy,half_z,yaw_steps,yaw_step_deg]:
the flags need --close-loops (or a join) and sane values, else the run ends with status 2 before any work; on the circle drive of
tests/test_close_loops_gpu.py the report's lines gain search_score guess_score runner_up_score search_used, and without the flag they
and every other output file stay what they are.

Measured on that drive (10 000-point scans of a sparse scene, submaps of three, pose-derived guesses within 0.1 m): the plain run closes
8 loop edges.  With a window of +-3 m and +-6 degrees, three of the eight candidate pairs keep their guess (3 235 of 4 096 points at the
guess, nothing better) and five are moved 2.5 to 3 m to a transform that scores 1 to 3 % above a guess of about 2 930 -- the ground lands
in occupied voxels wherever it is put, runner_up_score is as high as the pick -- and the ICP ends there with a score of 0.91, as good as
the right one's.  CheckResult then finds the edges of a frame apart and drops them all: 0 loop edges.  So what the wider window leaves
is printed and only its format is asserted; the one-candidate window is the case that has to equal the plain run."""
import json
import subprocess

import numpy as np
import pytest

from test_close_loops_gpu import LOOP_FLAGS, PERIOD, RADIUS, circle_drive  # noqa: F401


@pytest.fixture(scope="module")
def exe():
    from staticmapping_amd import build
    build.build()
    return build.build_shard_driver()


@pytest.mark.parametrize("flags", [["--loop-guess-search", "1"], ["--loop-guess-search", "0"], ["--loop-guess-resolution", "0.25"], ["--loop-guess-window", "10,1,5,2"]])
def test_the_flags_need_close_loops(exe, flags):
    r = subprocess.run([exe, "--scans", "/nonexistent-dir"] + flags, capture_output=True, text=True)
    assert r.returncode == 2 and "need --close-loops" in r.stderr and "--loop-guess-search" in r.stderr


@pytest.mark.parametrize("flags", [["--loop-guess-resolution", "0"], ["--loop-guess-resolution", "-1"], ["--loop-guess-resolution", "nan"], ["--loop-guess-window", "10,1,5"],
                                   ["--loop-guess-window", "-1,1,5,2"], ["--loop-guess-window", "10,-1,5,2"], ["--loop-guess-window", "10,1,-5,2"],
                                   ["--loop-guess-window", "10,1,5,inf"], ["--loop-guess-window", "wide"]])
def test_bad_values_are_refused_before_any_work(exe, flags):
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", "x.txt", "--loop-guess-search", "1"] + flags, capture_output=True, text=True)
    assert r.returncode == 2 and "bad guess search" in r.stderr


def test_good_values_get_as_far_as_the_scans(exe):
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", "x.txt", "--loop-guess-search", "1", "--loop-guess-resolution", "0.25",
                        "--loop-guess-window", "12,1,4,1.5"], capture_output=True, text=True)
    assert r.returncode == 2 and "cannot open" in r.stderr


@pytest.mark.gpu
def test_report_gains_the_scores_and_nothing_else_moves_without_the_flag(circle_drive, exe, tmp_path):  # noqa: F811
    seq, _ = circle_drive
    step = 2.0 * np.pi * RADIUS / PERIOD

    def run(tag, extra):
        files = {k: tmp_path / ("%s_%s.txt" % (k, tag)) for k in ("pose", "corrected", "report")}
        r = subprocess.run([exe, "--scans", seq, "--gpus", "1", "--batch", "8", "--iterations", "30", "--guess-tx", "%.4f" % step, "--guess", "ctrv",
                            "--out", str(files["pose"]), "--close-loops", str(files["corrected"]), "--loop-report", str(files["report"])] + LOOP_FLAGS + extra,
                           capture_output=True, text=True, timeout=600)
        print(r.stderr[-1500:])
        assert r.returncode == 0, r.returncode
        return files, json.loads(r.stdout.strip().splitlines()[-1])
    plain, line0 = run("plain", [])
    one, line_one = run("one", ["--loop-guess-search", "1", "--loop-guess-window", "0,0,0,2"])
    on, line1 = run("on", ["--loop-guess-search", "1", "--loop-guess-window", "6,1,3,2"])
    rows0 = [ln.split() for ln in plain["report"].read_text().splitlines()]
    rows_one = [ln.split() for ln in one["report"].read_text().splitlines()]
    rows1 = [ln.split() for ln in on["report"].read_text().splitlines()]
    print("loop edges: plain", line0["loop_edges"], "one candidate", line_one["loop_edges"], "13 x 13 x 3 x 7 candidates", line1["loop_edges"])
    print("report lines with the one-candidate window:", rows_one)
    print("report lines with the wider window:", rows1)
    assert line0["loop_edges"] >= 1 and len(rows0) == line0["loop_edges"] and all(len(r) == 4 for r in rows0)
    # a window of one candidate is the guess itself: never used, so the edges, the report's first four fields and the corrected poses
    # are the plain run's byte for byte, and the new fields say so
    assert [r[:4] for r in rows_one] == rows0 and all(len(r) == 8 for r in rows_one)
    assert plain["corrected"].read_bytes() == one["corrected"].read_bytes()
    for r in rows_one:
        search, guess, runner_up, used = (int(v) for v in r[4:])
        assert 0 < search == guess <= 4096 and runner_up == 0 and used == 0
    # the alignment run does not search
    assert plain["pose"].read_bytes() == one["pose"].read_bytes() == on["pose"].read_bytes()
    # the wider window: the format of whatever edges survive (see the module's docstring)
    assert len(rows1) == line1["loop_edges"] and all(len(r) == 8 for r in rows1)
    for r in rows1:
        search, guess, runner_up, used = (int(v) for v in r[4:])
        assert 0 < guess <= search <= 4096 and 0 <= runner_up <= search and used == int(search > guess)
