"""tests/cpp/test_statistic_removal.cc: the StatisticRemoval class and the opt-in Factory of include/smhip/filters.h, configured
from XML text.  Host side only: it needs the library (defaults, ConfigsValid()) and no GPU."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_statistic_removal.cc")


@pytest.fixture(scope="module")
def exe():
    from staticmapping_amd import _capi
    lib = _capi.library_path()
    assert os.path.exists(lib), "libsmhip.so has not been built"
    out = os.path.join(ROOT, "tests", "cpp", "_build", "test_statistic_removal")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    hdr = os.path.join(ROOT, "include", "smhip", "filters.h")
    if (not os.path.exists(out)) or max(os.path.getmtime(SRC), os.path.getmtime(hdr), os.path.getmtime(lib)) > os.path.getmtime(out):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", out,
                               "-L", os.path.dirname(lib), "-lsmhip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_cpp_statistic_removal(exe):
    out = subprocess.run([exe], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["failed"] == 0
    # the default Factory and Factory(true) still report the name as the reference does for an unknown one
    assert out.stderr.count("[XML] StatisticRemoval not supported yet.") == 4


def test_cpp_unknown_parameter_is_refused(exe):
    out = subprocess.run([exe, "unknown"], text=True, capture_output=True, timeout=120)
    assert out.returncode != 0 and "Check failed: all_right (param mean_k)" in out.stderr
    assert "failed" not in out.stdout
