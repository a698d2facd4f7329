"""smhip_shard --loop-huber K and --loop-report FILE without a GPU: both need --close-loops, a K that is negative or not finite is a bad
loop setting, and with everything in order the run gets as far as the scans.  All against a scan directory that does not exist."""
import subprocess

import pytest


@pytest.fixture(scope="module")
def exe():
    from staticmapping_amd import build
    build.build()
    return build.build_shard_driver()


def _run(exe, *flags):
    return subprocess.run([exe, "--scans", "/nonexistent-dir", *flags], capture_output=True, text=True)


def test_both_flags_need_close_loops(exe):
    r = _run(exe, "--loop-huber", "1")
    assert r.returncode == 2 and "--loop-huber needs --close-loops" in r.stderr
    r = _run(exe, "--loop-huber", "0")                         # also when it asks for nothing
    assert r.returncode == 2 and "--loop-huber needs --close-loops" in r.stderr
    r = _run(exe, "--loop-report", "r.txt")
    assert r.returncode == 2 and "--loop-report needs --close-loops" in r.stderr


@pytest.mark.parametrize("k", ["-1", "-0.5", "nan", "inf", "-inf", "one", "1x", ""])
def test_a_threshold_that_is_negative_or_not_finite_is_a_bad_loop_setting(exe, k):
    r = _run(exe, "--close-loops", "x.txt", "--loop-huber", k)
    assert r.returncode == 2 and "bad loop setting" in r.stderr and "--loop-huber" in r.stderr


@pytest.mark.parametrize("flags", [["--loop-huber", "1"], ["--loop-huber", "0"], ["--loop-huber", "2.5e0", "--loop-report", "r.txt"], ["--loop-report", "r.txt"]])
def test_flags_in_order_get_as_far_as_the_scans(exe, flags, tmp_path):
    r = subprocess.run([exe, "--scans", "/nonexistent-dir", "--close-loops", "x.txt", *flags], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 2 and "cannot open" in r.stderr
    assert not (tmp_path / "r.txt").exists() and not (tmp_path / "x.txt").exists()


def test_the_usage_names_the_flags(exe):
    r = _run(exe, "--no-such-flag")
    assert r.returncode == 2 and "--loop-huber" in r.stderr and "--loop-report" in r.stderr
