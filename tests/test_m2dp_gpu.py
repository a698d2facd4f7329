"""The device M2DP descriptor (smhip_m2dp_*, staticmapping_amd/m2dp.py, csrc/smhip_m2dp.hip) against the restatement of
descriptor::M2dp (tests/m2dp_ref.py), stage by stage.  Every case runs in a process of its own under a timeout
(tests/m2dp_gpu_cases.py), so that a fault there ends the case and not the session.

The clouds are synth.velodyne_scan scans: 4 099 points (no multiple of a workgroup size), 20 000 points (scan_pair('cfg2')), that
scan cut at 42 m and scaled by 6 (about a tenth of it beyond max_distance, nothing beyond 256 m), a device-built 3 x 20 000 submap
at voxel 0.1 and one 120 000-point scan.  PCA eigenvalue gaps (l1 - l2) / l1 and (l2 - l3) / l2 measured with the restatement:
4 099: 0.608 / 0.990; 20 000 scan a: 0.577 / 0.990, b: 0.600 / 0.989, c: 0.388 / 0.995; the cut and scaled scan: 0.512 / 0.990; the
submap: 0.679 / 0.991 -- all above 10 %, so the f64
eigenvectors of the device's Jacobi and of numpy agree to ~1e-12 and only the final cast to float can differ.

projection  projected3 within 1.6e-5 m of the restatement's (two float ulp at 100 m); kept equal except rows whose length is within
            1e-5 relative of max_distance
histogram   given the device's own projected points: A_lo <= A <= A_lo + F cell by cell (A_lo: the restatement's histogram of the
            samples that are not near a bin border, F: the flagged samples spread over their cell and its +-1 neighbours in l and
            t), every row of A sums to n_kept, at most 0.1 % of the samples flagged (restatement on the CPU: 254 of 1 280 000 =
            0.02 % on scan a).  Defaults on three clouds and t = 8, p = 2, q = 4, r = 0.5, max_distance = 50.
            Then the descriptor given the device's own A: within 1e-6 of numpy's f64 SVD of that A under the sign rule, both
            halves of norm 1 within 1e-6
big         the same on 120 000 points
same_bits   two calls give the same A and descriptor bits; smhip_m2dp_from_filter_output on a device-built submap equals
            smhip_m2dp_f32 on its downloaded rows bit for bit, and the workspace still hands out the same cloud
gate        scans a, b (scan_pair('cfg2')) and c (scene 7, pose (20, -15, 0) yaw 70 deg, scan seed 9), 20 000 points each: the
            device's scores agree with the restatement's within 4 x the restatement's own score change when every flagged sample is
            moved to its neighbouring bin (measured on the CPU: a-b 0.9989828, change 5.6e-6, bound 2.2e-5; a-c 0.9653421, change
            3.8e-6, bound 1.5e-5; the case computes both again).  At the KITTI config's m2dp_match_score 0.98 a-b passes and a-c
            does not; neither score is within 0.005 of it
refusals    every refusal returns its status and a message, leaves a descriptor computed before untouched and the resident cloud
            readable and unchanged
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(name, timeout):
    p = subprocess.run([sys.executable, os.path.join(HERE, "m2dp_gpu_cases.py"), name], capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:], file=sys.stderr)
    assert p.returncode == 0, (name, p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip().splitlines()[-1] == "ok " + name


def test_projection_equals_restatement():
    run_case("projection", 300)


def test_histogram_within_flagged_band_and_descriptor_equals_svd():
    run_case("histogram", 300)


def test_full_size_cloud():
    run_case("big", 300)


def test_same_bits_and_resident_submap():
    run_case("same_bits", 300)


def test_descriptor_gate_on_three_scans():
    run_case("gate", 300)


def test_refusals_touch_nothing():
    run_case("refusals", 300)
