"""The device pose-graph optimiser (smhip_pose_graph_optimize, one kernel launch per call) against tests/pose_graph_ref.py: stage by
stage through smhip_pose_graph_last, the result against the restatement's direct solve, the angle edge cases, bits and bounds, and
IsamOptimizer end to end on a returning drive.  The graphs are those of tests/pose_graph_cases.py, which test_pose_graph_cpp.py
also runs through the same loop compiled for the CPU."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_ref as ref
from staticmapping_amd import IcpFastHip, SmhipError, kitti, pose_graph, synth
from test_pose_graph_cpp import _build_exe

pytestmark = pytest.mark.gpu

# Result parity, in metres and in rotation-matrix entries.  Measured on the MI355X over every graph below: the largest
# difference to the restatement's direct solve was MEASURED_T / MEASURED_R.  The bound is ten times that, far below the 1e-9 m at
# which a difference would be a finding.  (Before the acceptance rule took the rounding of the cost into account, the direct solve
# rejected one step on n64 that the preconditioned solves accepted, and that graph alone differed by 2.8e-11 m.)
MEASURED_T, MEASURED_R = 7.9e-14, 4.9e-15
BOUND_T, BOUND_R = 10 * MEASURED_T, 10 * MEASURED_R


@pytest.fixture(scope="module")
def handle():
    m = IcpFastHip(device=0, max_source_points=1024, max_target_points=1024)
    yield m
    m.close()


def _run(handle, g, **kw):
    return pose_graph.optimize(handle, g["poses"], g["edges"], g["Z"], fixed=g["fixed"], **kw)


def _check_stats(g, stats, max_iterations=50):
    cap = 12 * ref.non_chain_edges(g["edges"]) + 64
    assert stats["stop"] in ("step", "cost"), stats
    assert stats["iterations"] == stats["accepted_steps"] + stats["rejected_steps"] < max_iterations
    assert stats["pcg_cap"] == cap and 0 < stats["pcg_max_iterations"] < cap
    assert stats["pcg_iterations"] <= stats["iterations"] * stats["pcg_max_iterations"]
    assert stats["levels"] == int(np.ceil(np.log2(len(g["poses"]))))
    assert stats["final_cost"] <= stats["initial_cost"]


@pytest.mark.parametrize("name", sorted(cases.stage_cases()) + sorted(cases.circle_cases()))
def test_stage_parity_through_the_last_hook(handle, name):
    """residuals, A, B, the gradient and M^-1 v of the first linearisation (tolerances: cases.check_stage_parity)"""
    g, _, _ = cases.reference(name)
    _run(handle, g, max_iterations=1)
    n, m = len(g["poses"]), len(g["edges"])
    v = cases.probe_vector(n)
    cases.check_stage_parity(g, pose_graph.last(handle, n, m, v), v)


@pytest.mark.parametrize("name", sorted(cases.circle_cases()) + sorted(cases.stage_cases()))
def test_result_parity_with_the_direct_solve(handle, name):
    g, want, st = cases.reference(name)
    poses, stats = _run(handle, g)
    dt, dr = cases.pose_difference(poses, want)
    ratio = cases.gradient_ratio(g, poses)
    print(name, "difference", dt, dr, "gradient ratio", ratio, stats, "restatement", st["stop"], st["accepted"], st["rejected"], st["costs"])
    assert dt <= BOUND_T and dr <= BOUND_R
    assert ratio < 1e-9
    cases.check_costs(stats, st)
    _check_stats(g, stats)
    assert (stats["accepted_steps"], stats["rejected_steps"], stats["damping"]) == (st["accepted"], st["rejected"], st["damping"])
    fx = g["fixed"].astype(bool)
    assert (poses[fx] == g["poses"][fx]).all()
    assert (poses[:, 3] == [0, 0, 0, 1]).all()
    if name.startswith("circle"):
        # the drive closes: the drift at the end is gone, and three loop edges cost the preconditioned solve under 30 iterations a step
        end = np.linalg.norm(poses[-1, :3, 3] - g["truth"][-1, :3, 3])
        start = np.linalg.norm(g["poses"][-1, :3, 3] - g["truth"][-1, :3, 3])
        print("end of the drive: %.3f m off before, %.3f m after" % (start, end))
        assert start > 2.5 and end < 0.1 * start
        assert stats["pcg_max_iterations"] < 30


@pytest.mark.parametrize("name", sorted(cases.angle_cases()))
def test_angle_edge_cases(handle, name):
    g, want, st = cases.reference(name)
    poses, stats = _run(handle, g)
    dt, dr = cases.pose_difference(poses, want)
    print(name, "difference", dt, dr, stats, "restatement", st["stop"], st["accepted"], st["rejected"])
    assert dt <= BOUND_T and dr <= BOUND_R
    cases.check_costs(stats, st)
    n, m = len(g["poses"]), len(g["edges"])
    lin = pose_graph.last(handle, n, m)
    rot = np.linalg.norm(lin["r"][:, :3] * ref.DEFAULT_SIGMAS[:3], axis=1)
    if name.startswith("near_pi"):
        gap = 1e-3 if name == "near_pi" else 1e-6
        assert np.pi - 2 * gap < rot[-1] < np.pi                   # the Log argument of the loop edge starts just below pi
        assert stats["final_cost"] < 0.5 * stats["initial_cost"]
    if name == "near_zero":
        assert 0 < rot.max() < 1e-8
    if name == "two_nodes":
        # one edge, one free pose: the minimum is the measurement itself.  What is left is the rounding of X_0 Z and of the Log:
        # ~ 4 eps |t| / sigma ~ 1e-13 per whitened entry, 1e-26 squared; 1e-24 for the six of them with margin
        assert stats["initial_cost"] > 1.0 and stats["final_cost"] < 1e-24
        assert np.abs(poses[1] - g["poses"][0] @ g["Z"][0]).max() < 1e-13
    if name == "triangle":
        # the contradiction is shared out: the cost stays well above zero and every edge carries some of it
        assert stats["final_cost"] > 1.0
        after = ref.linearize(poses, g["edges"], g["Z"])[0]
        assert (np.abs(after).max(axis=1) > 0.1).all()
    if name in ("near_pi", "near_pi_6", "near_zero", "two_nodes"):
        cases.check_stage_parity(g, pose_graph.last(handle, n, m, cases.probe_vector(n)), cases.probe_vector(n))


def test_more_nodes_than_threads(handle):
    """1 500 nodes on 1 024 threads: the strided loops take a second round, 11 levels.  Against the restatement's sparse direct solve;
    the same bound as above scaled by the graph's extent would be kinder, but the plain one is asserted."""
    g, want, st = cases.large_circle()
    poses, stats = _run(handle, g)
    dt, dr = cases.pose_difference(poses, want)
    print("difference", dt, dr, "gradient ratio", cases.gradient_ratio(g, poses), stats, "restatement", st["stop"], st["accepted"], st["rejected"])
    assert dt <= 1e-9 and dr <= 1e-9                               # (measured: printed above; 1e-9 m is where a difference is a finding)
    assert cases.gradient_ratio(g, poses) < 1e-9
    cases.check_costs(stats, st)
    _check_stats(g, stats)
    with pytest.raises(SmhipError):
        pose_graph.last(handle, len(g["poses"]) - 1, len(g["edges"]))   # sizes other than the last call's are refused, nothing written


def test_two_calls_give_the_same_bits(handle):
    g, _, _ = cases.reference("circle240")
    a, sa = _run(handle, g)
    other, _, _ = cases.reference("n65")
    _run(handle, other)                                            # another graph in between leaves nothing behind
    b, sb = _run(handle, g)
    assert a.tobytes() == b.tobytes()
    assert sa == sb


def test_refused_calls_leave_the_poses_untouched_and_launch_nothing(handle):
    g, _, _ = cases.reference("n5")
    P, F, E, Z, _ = pose_graph._arrays(g["poses"], g["fixed"], g["edges"], g["Z"], None)
    lib = handle._lib

    def call(P, F, E, Z, n=None, m=None):
        before = P.tobytes()
        st = lib.smhip_pose_graph_optimize(handle._h, len(P) if n is None else n, pose_graph._ptr(P, pose_graph._capi.c_double_p),
                                           pose_graph._ptr(F, pose_graph.c_uint8_p), len(E) if m is None else m,
                                           pose_graph._ptr(E, pose_graph._capi.c_int32_p), pose_graph._ptr(Z, pose_graph._capi.c_double_p), None, None, None)
        assert st == 0 or P.tobytes() == before
        return st
    assert call(P.copy(), F, E, Z) == 0
    invalid, capacity = 1, 7
    bad = E.copy()
    bad[-1] = (4, 5)
    assert call(P.copy(), F, bad, Z) == invalid                    # an index out of range
    bad = E.copy()
    bad[0] = (1, 1)
    assert call(P.copy(), F, bad, Z) == invalid
    bad = Z.copy()
    bad[2, 3, 1] = np.inf
    assert call(P.copy(), F, E, bad) == invalid
    bad = P.copy()
    bad[3, 0, 0] += 1e-5
    assert call(bad, F, E, Z) == invalid                           # 1e-5 from orthonormal
    assert call(P.copy(), np.zeros_like(F), E, Z) == invalid       # no fixed node
    with pytest.raises(SmhipError):
        _run(handle, dict(g, fixed=np.zeros(5, np.uint8)))
    with pytest.raises(SmhipError):
        _run(handle, g, max_iterations=0)
    # one above either limit: decided from the sizes alone (the arrays are far shorter than the sizes claim, and nothing reads them)
    assert call(P.copy(), F, E, Z, n=pose_graph.MAX_NODES + 1) == capacity
    assert call(P.copy(), F, E, Z, m=pose_graph.MAX_EDGES + 1) == capacity
    # and the handle still works
    poses, stats = _run(handle, g)
    assert stats["stop"] in ("step", "cost")


def test_a_step_limit_is_reported(handle):
    g, want, _ = cases.reference("circle64")
    poses, stats = _run(handle, g, max_iterations=2)
    assert stats["stop"] == "max_iterations" and stats["iterations"] == 2
    assert stats["final_cost"] < stats["initial_cost"]
    assert cases.pose_difference(poses, want)[0] > 1e-6            # not there yet


def test_per_edge_sigmas_reach_the_kernel(handle):
    """a loop edge with sigmas a thousand times the others' barely pulls: the result is the restatement's with the same sigmas"""
    g, _, _ = cases.reference("n5")
    sig = np.tile(ref.DEFAULT_SIGMAS, (len(g["edges"]), 1))
    sig[-2] *= 1000.0
    want, st = ref.optimize(g["poses"], g["fixed"], g["edges"], g["Z"], sigmas=sig)
    poses, stats = _run(handle, g, sigmas=sig)
    dt, dr = cases.pose_difference(poses, want)
    print("difference", dt, dr)
    assert dt <= BOUND_T and dr <= BOUND_R
    cases.check_costs(stats, st)
    assert cases.pose_difference(poses, cases.reference("n5")[1])[0] > 1e-4


def returning_drive():
    """test_loop_detector_gpu.py's drive: 18 scans, six submaps of three -- three along a line, one 36 m away, two back on the first"""
    xs = [(0.8 * k, 0.03 * k, 0.6 * k) for k in range(9)]
    xs += [(30 + 0.8 * k, 20.0, 5.0) for k in range(3)]
    xs += [(0.3 + 0.8 * k, 0.4, 2.0) for k in range(6)]
    return [synth.make_pose(t=(x, y, 0.0), rpy_deg=(0, 0, yaw)) for x, y, yaw in xs]


def test_isam_optimizer_pulls_a_drifted_returning_leg_back():
    """The returning leg (submaps 4 and 5) is fed with 0.5 m and 0.5 degrees of drift.  After IsamOptimizer has seen all six submaps
    (loop edges from the detector on the sixth), the returning submaps stand closer to the ground truth than the drift put them:
    the factor left is reported and must be below 0.5 -- the matcher's own error decides the rest."""
    truth = returning_drive()
    drift = synth.make_pose(t=(0.3, 0.4, 0.0), rpy_deg=(0, 0, 0.5))                  # 0.5 m, 0.5 degrees
    fed = [P if k < 12 else drift @ P for k, P in enumerate(truth)]
    scene = synth.make_scene(0)
    with tempfile.TemporaryDirectory() as d:
        for k, P in enumerate(truth):
            kitti.write_bin(os.path.join(d, "%06d.bin" % k), synth.velodyne_scan(scene, P, seed=300 + k, n_points=20_000))
        np.savetxt(os.path.join(d, "poses.txt"), np.stack(fed).reshape(len(fed), 16), fmt="%.17g")
        out = subprocess.run([_build_exe(), "gpu", d, str(len(fed)), "3", "0.98"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:])
    print(out.stderr[-3000:])
    assert out.returncode == 0, out.returncode
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["loop_edges"] >= 2 and res["stop_reason"] in (1, 2)
    poses = np.array(res["poses"]).reshape(6, 4, 4)
    for s in (4, 5):
        before = np.linalg.norm(fed[3 * s][:3, 3] - truth[3 * s][:3, 3])
        after = np.linalg.norm(poses[s][:3, 3] - truth[3 * s][:3, 3])
        print("submap %d: %.3f m from the truth as fed, %.3f m after, factor %.3f" % (s, before, after, after / before))
        assert before > 0.45 and after < 0.5 * before
    assert np.abs(poses[0] - truth[0]).max() == 0.0                                 # the first submap is the gauge
    # UpdateInnerFramePose: the last submap's frames moved with it
    frames = np.array(res["last_frame_poses"]).reshape(3, 4, 4)
    for i in range(3):
        want = poses[5] @ np.linalg.inv(fed[15]) @ fed[15 + i]
        assert np.abs(frames[i] - want).max() < 1e-9
