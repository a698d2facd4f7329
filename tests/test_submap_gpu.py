"""The device submap build (smhip_submap_build_f32, smhip_filter_output_to_target, staticmapping_amd/submap.py) against the
restatement of Submap::InsertFrame (tests/submap_ref.py) and the oracle.  Every case runs in a process of its own under a
timeout (tests/submap_gpu_cases.py), so that a fault there ends the case and not the session.

cloud      the device cloud equals the restatement bit for bit, rows and source_index: 3 x 20 000-point frames of the straight
           drive at voxel 0.1 and 0, stride 4 and 5, unequal frames with an empty one; and equals what the host transform followed
           by smhip_filter_chain_f32([VoxelGrid]) returns
big        the same for 5 x 120 000 points at voxel 0.1 on a handle with max_target_points 2^20
handover   smhip_filter_output_to_target = smhip_prepare_target_f32 on the downloaded rows (size, points, normals, bit for bit);
           output_to_source followed by get_source returns the cloud; NOT_READY without a cloud
refusals   every refusal returns its status, sets a message and leaves the cloud built before readable and unchanged
matching   two device-built 3-scan submaps at voxel 0.1, source on target from a guess 0.25 m / 0.05 m off the truth, against
           cref.icp_fast_align on the restated clouds with the oracle's normals: 1e-4 rad, 1e-3 m, score 1e-4 (the CPU oracle
           alone: score 0.9005 in 6 iterations, 5.6e-5 rad / 7.6e-4 m from the truth).  The same pair through C++ Submap and
           ConnectSubmaps (tests/cpp/test_submap.cc) equals the Python path that does what ConnectSubmaps does -- Cloud() of both
           submaps with the host CalculateNormals, IcpFast as a batch of one -- to 1e-9 rad and 1e-9 m
driver     smhip_shard --gpus 1 --submap-frames 3 --submap-edges on 12 generated scans: three edges, each against the oracle on submaps
           restated from the pose file as written (same tolerance plus the file's printed precision), accepted = score >= 0.7.  A
           trailing group that is not full is dropped: with --batch 1 (every pair aligned on its own, so the pose files agree line
           for line) 13 scans give the same three edges as 12, text for text; 11 scans hold three full groups only, so they give
           the first two of those edges, not three
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def run_case(name, timeout):
    p = subprocess.run([sys.executable, os.path.join(HERE, "submap_gpu_cases.py"), name], capture_output=True, text=True, timeout=timeout)
    print(p.stdout)
    print(p.stderr[-4000:], file=sys.stderr)
    assert p.returncode == 0, (name, p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert p.stdout.strip().splitlines()[-1] == "ok " + name


def test_cloud_equals_restatement_and_composition():
    run_case("cloud", 600)


def test_full_size_submap_equals_restatement():
    run_case("big", 900)


def test_hand_over_to_target_and_source():
    run_case("handover", 600)


def test_refusals_leave_the_resident_cloud():
    run_case("refusals", 300)


def test_device_built_submaps_match_like_the_oracle():
    run_case("matching", 600)


def test_driver_writes_the_edges_of_consecutive_submaps():
    run_case("driver", 900)
