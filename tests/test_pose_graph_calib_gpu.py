"""The device pose-graph optimiser with HANDEYE factors (smhip_pose_graph_optimize_calib, one kernel launch per call) against
tests/pose_graph_calib_ref.py on the graphs of tests/pose_graph_calib_cases.py, each with the calibration held and free: the first
linearisation through smhip_pose_graph_last, the result against the restatement's direct solve, the same stop reason, counts and
damping, the longest conjugate-gradient solve, bits, refusals, and 1 100 nodes with a factor each against scipy's sparse LU."""
import numpy as np
import pytest

import pose_graph_calib_cases as cases
import pose_graph_calib_ref as calib
import pose_graph_cases as base
import pose_graph_gps_cases as gps_cases
import pose_graph_robust_cases as robust_cases
from staticmapping_amd import IcpFastHip, SmhipError, pose_graph

pytestmark = pytest.mark.gpu

# Result parity, in metres and in rotation-matrix entries.  The bound of a graph is ten times the restatement's own direct-against-PCG
# disagreement on it (the project's standing rule; where the two agree to the bit, the rounding of the largest coordinate, 1e-15 |t|).
# Measured on the MI355X over the twenty small graphs: the largest difference to the restatement's direct solve was MEASURED_T (ring64_free,
# whose own two solves differ by 1.4e-14 m) / MEASURED_R (gps24_free); a second bound is ten times that.  The drives of 1 100 nodes:
# MEASURED_LARGE_T (free; its own sparse-LU and sparse-PCG solves differ by 2.8e-14 m) / MEASURED_LARGE_R (held).  The longest
# conjugate-gradient solve was the restatement's PCG count to the iteration on all twenty-two.
MEASURED_T, MEASURED_R = 6.5e-14, 7.2e-15
MEASURED_LARGE_T, MEASURED_LARGE_R = 2.4e-14, 9.4e-16
STAGE = ["chain1_free", "chain2_held", "chain4_free", "chain62_free", "chain63_held", "chain63_free", "chain64_free", "ring16_free", "gps24_free"]


@pytest.fixture(scope="module")
def handle():
    m = IcpFastHip(device=0, max_source_points=1024, max_target_points=1024)
    yield m
    m.close()


def _run(handle, g, entry=pose_graph.optimize_calib, **kw):
    a = {**dict(huber=g["huber"]), **kw}
    return entry(handle, g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"], **a)


@pytest.mark.parametrize("name", STAGE)
def test_stage_parity(handle, name):
    """residuals, A and B within 1e-12 relative, the gradient and M^-1 v by pose_graph_gps_cases.check_stage_parity's rules, at the
    sizes around a level of the cyclic reduction, with the calibration node adjacent to the last chain node (a chain block) and
    with both extra vertices"""
    g = cases.graph(name)
    _run(handle, g, max_iterations=1)
    n, m = len(g["poses"]), len(g["kinds"])
    v = base.probe_vector(n)
    cases.check_stage_parity(g, pose_graph.last(handle, n, m, v), v)


@pytest.mark.parametrize("name", cases.names())
def test_result_parity(handle, name):
    g, want, st = cases.reference(name)
    _, _, sp = cases.reference(name, "pcg")
    same, own, ratio_ref = cases.qualifies(name)
    assert same and own < 1e-10 and ratio_ref < 1e-9
    poses, stats = _run(handle, g)
    dt, dr = base.pose_difference(poses, want)
    floor = 1e-15 * np.abs(want[:, :3, 3]).max()          # (a disagreement of exactly 0 -- chains of 1 and 2 nodes -- leaves the rounding of one entry)
    print(name, "difference", dt, dr, "restatement's direct against PCG", own, "bound", 10 * max(own, floor), stats, "restatement", st["stop"], st["accepted"], st["rejected"],
          st["damping"], "longest solve: device", stats["pcg_max_iterations"], "restatement", sp["pcg_max"])
    assert max(dt, dr) <= 10 * max(own, floor)
    assert dt <= 10 * MEASURED_T and dr <= 10 * MEASURED_R
    assert cases.gradient_ratio(g, poses) < 1e-9
    base.check_costs(stats, st)
    assert (stats["stop_reason"], stats["accepted_steps"], stats["rejected_steps"], stats["damping"]) == (st["stop"], st["accepted"], st["rejected"], st["damping"])
    assert stats["pcg_cap"] == 12 * calib.non_chain_edges(g) + 64
    assert abs(stats["pcg_max_iterations"] - sp["pcg_max"]) <= max(2, 0.1 * sp["pcg_max"])
    fx = g["fixed"].astype(bool)
    assert (poses[fx] == g["poses"][fx]).all() and (poses[:, 3] == [0, 0, 0, 1]).all()
    rep = pose_graph.last_robust(handle, len(g["kinds"]))                # the report serves the new entry
    robust_cases.check_report_parity(g, (rep["norm"], rep["weight"], rep["cost"]), calib.report(g, want))


@pytest.mark.parametrize("free", [False, True])
def test_more_factors_than_threads(handle, free):
    """1 100 nodes, 2 199 (2 200) factors on 1 024 threads, a calibration node of degree 1 100 (1 101): against the restatement's sparse
    direct solve, which its own sparse PCG solve follows within 1e-10 with the same counts"""
    g, want, st = cases.large_drive(free)
    same, own, own_pcg = st["own"]
    assert same and own < 1e-10 and cases.gradient_ratio(g, want) < 1e-9
    poses, stats = _run(handle, g)
    dt, dr = base.pose_difference(poses, want)
    print("free" if free else "held", "difference", dt, dr, "restatement's direct against PCG", own, "longest solve: device", stats["pcg_max_iterations"], "restatement", own_pcg,
          stats, "restatement", st["stop"], st["accepted"], st["rejected"], "worst position error", cases.truth_error(g, g["poses"]), "->", cases.truth_error(g, poses))
    assert max(dt, dr) <= 10 * own
    assert dt <= 10 * MEASURED_LARGE_T and dr <= 10 * MEASURED_LARGE_R
    base.check_costs(stats, st)
    assert (stats["stop_reason"], stats["accepted_steps"], stats["rejected_steps"], stats["damping"]) == (st["stop"], st["accepted"], st["rejected"], st["damping"])
    assert stats["pcg_cap"] == 12 * calib.non_chain_edges(g) + 64
    assert abs(stats["pcg_max_iterations"] - own_pcg) <= max(2, 0.1 * own_pcg)
    assert cases.truth_error(g, poses) < cases.truth_error(g, g["poses"])


def test_two_calls_give_the_same_bits(handle):
    g = cases.graph("ring64_free")
    a, sa = _run(handle, g)
    la = pose_graph.last(handle, len(g["poses"]), len(g["kinds"]), base.probe_vector(len(g["poses"])))
    _run(handle, cases.graph("chain23_held"))                            # another graph in between leaves nothing behind
    b, sb = _run(handle, g)
    lb = pose_graph.last(handle, len(g["poses"]), len(g["kinds"]), base.probe_vector(len(g["poses"])))
    assert a.tobytes() == b.tobytes() and sa == sb and all(la[key].tobytes() == lb[key].tobytes() for key in la)


@pytest.mark.parametrize("name", ["robust16", "robust_point"])
def test_without_a_handeye_the_bytes_are_the_robust_entrys(handle, name):
    g = robust_cases.graph(name)
    n, m = len(g["poses"]), len(g["kinds"])
    want, sw = _run(handle, g, entry=pose_graph.optimize_robust)
    lw = pose_graph.last(handle, n, m, base.probe_vector(n))
    rw = pose_graph.last_robust(handle, m)
    got, sg = _run(handle, g)
    lg = pose_graph.last(handle, n, m, base.probe_vector(n))
    rg = pose_graph.last_robust(handle, m)
    assert got.tobytes() == want.tobytes() and sg == sw
    assert all(lg[key].tobytes() == lw[key].tobytes() for key in lw) and all(rg[key].tobytes() == rw[key].tobytes() for key in rw)


def test_refused_calls_leave_the_poses_and_the_handle(handle):
    g = cases.graph("chain4_free")
    before = np.array(g["poses"]).tobytes()
    he = int(np.flatnonzero(g["kinds"] == calib.HANDEYE)[0])
    pr = int(np.flatnonzero(g["kinds"] == calib.PRIOR)[0])
    e = g["ij"].copy()
    e[he] = (2, 2)
    d = g["data"].copy()
    d[he, 0] += 1e-3
    keep = [k for k in range(len(g["kinds"])) if k != pr]
    for match, change in (("hand-eye factor that joins a node to itself", dict(ij=e)), ("odometer pose", dict(data=d)),
                          ("calibration node of a hand-eye factor and has no prior", dict(keep=keep))):
        a = dict(poses=g["poses"], kinds=g["kinds"], ij=g["ij"], data=g["data"], sigmas=g["sigmas"], huber=g["huber"])
        a.update({k: v for k, v in change.items() if k != "keep"})
        if "keep" in change:
            a.update({k: a[k][keep] for k in ("kinds", "ij", "data", "sigmas", "huber")})
        with pytest.raises(SmhipError, match=match):
            pose_graph.optimize_calib(handle, a["poses"], a["kinds"], a["ij"], a["data"], fixed=g["fixed"], sigmas=a["sigmas"], huber=a["huber"])
        assert np.array(g["poses"]).tobytes() == before
    for entry in (pose_graph.optimize_robust, lambda *a, huber=None, **kw: pose_graph.optimize_factors(*a, **kw)):      # the older entries: kind 3 stays refused
        with pytest.raises(SmhipError, match="none of BETWEEN, PRIOR and POINT"):
            _run(handle, g, entry=entry)
    poses, stats = _run(handle, g)
    assert stats["stop"] in ("step", "cost")


def test_isam_optimizer_with_use_odom_on_the_device(tmp_path):
    """the AddDetected sequence of test_pose_graph_calib_cpp.py without the Solver hook: the same assertions, and the poses of its CPU run"""
    import test_pose_graph_calib_cpp as cpp
    g_held, g_free = cases.graph("ring16_held"), cases.graph("ring16_free")
    runs = {}
    for where in ("gpu", "host"):
        runs[where] = (cpp.run_isam(where, tmp_path, g_held, 1, 0), cpp.run_isam(where, tmp_path, g_free, 1, 1), cpp.run_isam(where, tmp_path, g_held, 0, 0))
    cpp.check_isam(g_held, g_free, *runs["gpu"], device=True)
    for dev, host in zip(runs["gpu"], runs["host"]):
        dt, dr = base.pose_difference(dev["poses"], host["poses"])
        print("device against the CPU run", dt, dr, "calibration", np.abs(dev["tf"] - host["tf"]).max())
        assert dt < 1e-9 and dr < 1e-9 and np.abs(dev["tf"] - host["tf"]).max() < 1e-9
