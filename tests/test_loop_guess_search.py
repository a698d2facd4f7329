"""LoopDetectorSettings::guess_search of include/smhip/back_end.h (tests/cpp/test_loop_guess_search.cc).

host  no GPU: a scan matcher that records where its Align starts and a hook in place of the device search (SetGuessSearcher, the
      SetSolver pattern) -- the searched guess is used only when best_score > guess_score, the new LoopEdge fields are filled,
      init_guess stays the pose-derived one, a refused search fails the pair, and with guess_search off no search is called and the
      edge is what it was.
gpu   CloseLoop on the experiment's pair (tests/guess_search_cases.py: 7.6 m of drift) with the drifted poses.  With guess_search on the
      edge has to be within 0.1 m and 0.01 in the rotation entries of the truth (the bound tests/test_loop_detector_gpu.py uses for
      edges), search_used set and best_score > guess_score.  The same call with guess_search off is run once and its error printed, not
      asserted: the device matcher (f32, epsilon-approximate search) may end elsewhere than the CPU oracle, which ends 1.17 m off."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import guess_search_cases as cases
from staticmapping_amd import kitti

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_loop_guess_search.cc")


def _build_exe():
    from staticmapping_amd import build
    lib = build.build()
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "test_loop_guess_search")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    hdrs = [os.path.join(ROOT, "include", "smhip", h) for h in ("back_end.h", "m2dp.h", "registrator.h", "edge_information.h")] + [os.path.join(ROOT, "include", "smhip.h")]
    if (not os.path.exists(exe)) or max([os.path.getmtime(SRC), os.path.getmtime(lib)] + [os.path.getmtime(h) for h in hdrs]) > os.path.getmtime(exe):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                               "-L", os.path.dirname(lib), "-lsmhip", "-Wl,-rpath," + os.path.dirname(lib),
                               "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return exe


def test_search_step_of_close_loop_on_the_host():
    out = subprocess.run([_build_exe(), "host"], text=True, capture_output=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout


@pytest.mark.gpu
def test_close_loop_recovers_the_drifted_pair_with_the_search_on():
    target, source, truth, guess = cases.experiment()
    pose_t = np.eye(4)
    pose_t[:3, 3] = (40.0, -12.0, 0.0)
    with tempfile.TemporaryDirectory() as d:
        kitti.write_bin(os.path.join(d, "target.bin"), target)
        kitti.write_bin(os.path.join(d, "source.bin"), source)
        np.savetxt(os.path.join(d, "poses.txt"), np.stack([pose_t, pose_t @ guess]).reshape(2, 16), fmt="%.17g")
        out = subprocess.run([_build_exe(), "gpu", d], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    print(out.stderr[-3000:])
    assert out.returncode == 0, out.returncode
    res = json.loads(out.stdout.strip().splitlines()[-1])
    err = {}
    for k in ("on", "off"):
        T = np.array(res["transform_" + k]).reshape(4, 4)
        err[k] = (float(np.linalg.norm(T[:3, 3] - truth[:3, 3])), float(np.abs(T[:3, :3] - truth[:3, :3]).max()))
        print("guess_search %s: accepted %s, -log(score) %.6f, translation error %.4f m, rotation entries %.5f" %
              (k, res["accepted_" + k], res["score_" + k], err[k][0], err[k][1]))
    print("search", res["search_score"], "at the guess", res["guess_score"], "runner-up", res["runner_up_score"])
    assert np.abs(np.array(res["init_guess"]).reshape(4, 4) - guess).max() < 1e-9          # init_guess stays the pose-derived one
    assert res["accepted_on"] and res["search_used"] and res["search_score"] > res["guess_score"]
    assert err["on"][0] < 0.1 and err["on"][1] < 0.01
    assert res["off_untouched"]
