"""back_end::LoopDetector on the device (tests/cpp/test_loop_detector.cc, mode `gpu`): a generated drive that returns to its start,
six submaps of 3 x 20 000 points at voxel 0.1 -- three along a straight line, one 36 m away, two back on the first ones -- with
their device descriptors (Submap::CalculateDescriptor on the resident cloud), use_descriptor on at the KITTI config's
m2dp_match_score 0.98 and loop_ignore_threshold 2.  The restatement on the CPU scores the returning submaps 0.9946 .. 0.9998
against the ones they revisit and the far one 0.960 .. 0.968 against all.  The detector is in kEnteringLoop after the fifth submap
and in kContinousLoop after the sixth, whose candidates are the pairs (0, 5), (1, 5), (2, 5); its edges equal CloseLoop called
directly on those pairs with a matcher of its own each, bit for bit."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

from staticmapping_amd import kitti, synth
from test_loop_detector_cpp import _build_exe

pytestmark = pytest.mark.gpu


def track():
    xs = [(0.8 * k, 0.03 * k, 0.6 * k) for k in range(9)]
    xs += [(30 + 0.8 * k, 20.0, 5.0) for k in range(3)]
    xs += [(0.3 + 0.8 * k, 0.4, 2.0) for k in range(6)]
    return [synth.make_pose(t=(x, y, 0.0), rpy_deg=(0, 0, yaw)) for x, y, yaw in xs]


def test_returning_drive_reaches_continous_loop_and_edges_equal_close_loop():
    poses = track()
    scene = synth.make_scene(0)
    with tempfile.TemporaryDirectory() as d:
        for k, P in enumerate(poses):
            kitti.write_bin(os.path.join(d, "%06d.bin" % k), synth.velodyne_scan(scene, P, seed=300 + k, n_points=20_000))
        np.savetxt(os.path.join(d, "poses.txt"), np.stack(poses).reshape(len(poses), 16), fmt="%.17g")
        out = subprocess.run([_build_exe(), "gpu", d, str(len(poses)), "3", "0.98"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    print(out.stderr[-3000:])
    assert out.returncode == 0, out.returncode
    res = json.loads(out.stdout.strip().splitlines()[-1])
    no_loop, entering, continous = 0, 2, 3                      # LoopStatus, loop_detector.h:41-47
    assert res["status"] == [no_loop] * 4 + [entering, continous]
    assert res["last_status_before"] == entering                # the result carries the status before the frame
    assert res["pairs"] == [[0, 5], [1, 5], [2, 5]]
    assert min(res["scores"][:3]) > 0.985 and res["scores"][3] < 0.975
    assert res["edges_equal_direct"] is True and res["direct_edges"] == len(res["edges"]) >= 2
    for e in res["edges"]:
        want = np.linalg.inv(poses[3 * e["target"]]) @ poses[3 * e["source"]]
        got = np.array(e["transform"]).reshape(4, 4)
        assert np.abs(got[:3, 3] - want[:3, 3]).max() < 0.1 and np.abs(got[:3, :3] - want[:3, :3]).max() < 0.01, e
    print("CheckResult on these edges:", res["close_succeed"])  # (its limits are checked on hand-made edges, test_loop_detector_cpp.py)
