"""tests/cpp/test_ground_filters.cc: GroundRemoval, GroundRemoval2 and RangeImage through include/smhip/filters.h."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ground_filters.cc")


def test_ground_filters_program_compiles_without_a_gpu():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), SRC])


@pytest.mark.gpu
def test_cpp_ground_filters():
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_ground_filters")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    hdr = os.path.join(ROOT, "include", "smhip", "filters.h")
    if (not os.path.exists(exe)) or max(os.path.getmtime(SRC), os.path.getmtime(hdr), os.path.getmtime(lib)) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                               "-L", os.path.dirname(lib), "-lsmhip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], text=True, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["failed"] == 0
