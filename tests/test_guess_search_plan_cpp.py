"""tests/cpp/test_guess_search_plan.cc: staticmapping_amd/csrc/guess_search_plan.h on the host, without a GPU -- every refusal the guess
search decides from its sizes alone, the candidate and bitmap sizes at and one past each limit, the packed voxel layout, the sample
rule, the yaw transform and the pick rule on hand-made volumes.  Its pick is also held against the restatement's on random volumes."""
import os
import subprocess

import numpy as np

import guess_search_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_guess_search_plan.cc")
HEADER = os.path.join(ROOT, "staticmapping_amd", "csrc", "guess_search_plan.h")


def _build_exe():
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_guess_search_plan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if (not os.path.exists(exe)) or max(os.path.getmtime(SRC), os.path.getmtime(HEADER)) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", SRC, "-o", exe])
    return exe


def test_plan_header_compiles_alone_as_host_code(tmp_path):
    alone = tmp_path / "alone.cc"
    alone.write_text('#include "%s"\nint main() { return smhip_guess_search::kMaxCandidates == (1LL << 25) ? 0 : 1; }\n' % HEADER)
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", str(alone)])


def test_refusals_limits_layout_and_pick_rule():
    out = subprocess.run([_build_exe()], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


def test_pick_equals_the_restatement_on_random_volumes(tmp_path):
    rng = np.random.default_rng(0)
    for k, (hxy, hz, ky, top) in enumerate([(3, 1, 2, 3), (0, 0, 0, 5), (5, 0, 1, 2), (1, 2, 3, 1), (4, 1, 0, 4)]):
        volume = rng.integers(0, top + 1, (2 * ky + 1, 2 * hz + 1, 2 * hxy + 1, 2 * hxy + 1)).astype("<i4")       # many ties
        path = tmp_path / ("volume%d.bin" % k)
        path.write_bytes(volume.tobytes())
        out = subprocess.run([_build_exe(), "pick", str(path), str(hxy), str(hz), str(ky)], text=True, capture_output=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        (a, i, j, kk), best, runner_up = ref.pick(volume, hxy, hz, ky)
        assert out.stdout.split() == [str(v) for v in (a, i, j, kk, best, runner_up)]
