"""tests/cpp/test_map_package.cc: include/smhip/map_package.h without a GPU -- PlanMapPackage against the restatement
(tests/map_package_ref.py) exactly, the description file and its failure mode, and a package into a missing directory."""
import os
import subprocess

import numpy as np
import pytest

import map_package_cases as cases
import map_package_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_map_package.cc")


def _build_exe():
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_map_package")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    deps = [os.path.join(ROOT, "include", "smhip", h) for h in ("map_package.h", "mrvm.h", "pcd.h", "registrator.h")]
    deps += [os.path.join(ROOT, "include", "smhip.h"), SRC, lib]
    if (not os.path.exists(exe)) or max(os.path.getmtime(d) for d in deps) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                               "-L", os.path.dirname(lib), "-lsmhip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def _case_file(tmp_path, t, border, width):
    path = tmp_path / "case.bin"
    t = np.asarray(t, "<f8").reshape(-1, 3)
    path.write_bytes(np.array([len(t), border, width], "<f8").tobytes() + t.tobytes())
    return str(path)


def _run(args):
    out = subprocess.run([_build_exe()] + args, text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def test_header_compiles_alone(tmp_path):
    alone = tmp_path / "alone.cc"
    alone.write_text('#include "smhip/map_package.h"\nint main() { smhip::MapPackageOptions o; return o.enable ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), str(alone)])


@pytest.mark.parametrize("name", sorted(cases.plan_cases()))
def test_plan_equals_the_restatement(name, tmp_path):
    t, border, width = cases.plan_cases()[name]
    want = ref.plan(t, border, width)
    lines = _run(["plan", _case_file(tmp_path, t, border, width)]).strip().splitlines()
    assert lines[0] == "steps %d %d" % (want["x_steps"], want["y_steps"])
    assert len(lines) == 1 + len(want["pieces"])
    for text, p in zip(lines[1:], want["pieces"]):
        w = text.split()
        assert w[0] == "piece" and (int(w[1]), int(w[2])) == (p["x"], p["y"])
        assert tuple(float(v) for v in w[3:9]) == p["centre"] + p["bb_min"] + p["bb_max"]        # %.17g: the same doubles
        assert int(w[9]) == len(p["members"]) and [int(v) for v in w[10:]] == p["members"]


@pytest.mark.parametrize("name", sorted(cases.refused_cases()))
def test_refusals(name, tmp_path):
    t, border, width, by_reference = cases.refused_cases()[name]
    out = _run(["plan", _case_file(tmp_path, t, border, width)])
    assert out.startswith("refused ") and len(out.strip()) > len("refused ") + 5
    assert ("No good bounding box" in out) == by_reference


def test_description_file_and_its_failure_mode(tmp_path):
    t, border, width = cases.plan_cases()["walk"]
    out = _run(["xml", _case_file(tmp_path, t, border, width), str(tmp_path)])
    assert "all checks passed" in out, out
    assert (tmp_path / "map_package.xml").read_text() == ref.xml_text(ref.plan(t, border, width), "part_")
    assert sorted(os.listdir(tmp_path)) == ["case.bin", "empty.pcd", "map_package.xml"]


def test_package_into_a_missing_directory_leaves_nothing(tmp_path):
    out = _run(["save", str(tmp_path)])
    assert "all checks passed" in out, out
    assert os.listdir(tmp_path) == []
