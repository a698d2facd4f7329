"""The device pose-graph optimiser with Huber thresholds (smhip_pose_graph_optimize_robust, one kernel launch per call, and the report
of smhip_pose_graph_last_robust) against tests/pose_graph_robust_ref.py: the first linearisation's weighted rows through
smhip_pose_graph_last, the result against the restatement's direct (robust1500: sparse) solve, the report at the result, bits, and
IsamOptimizer with loop_closure_huber on the device.  The graphs are those of tests/pose_graph_robust_cases.py: rings of 16, 64, 65, 240
and 1 500 nodes with one or two wrong loop edges and the threshold 1 on the loop edges, and a GPS chain with one fix 5 m off and the
threshold on the POINT factors."""
import numpy as np
import pytest

import pose_graph_cases as base
import pose_graph_gps_ref as gps
import pose_graph_ref as ref
import pose_graph_robust_cases as cases
from staticmapping_amd import IcpFastHip, SmhipError, pose_graph

pytestmark = pytest.mark.gpu

# Result parity, in metres and in rotation-matrix entries.  Before measurement the bound was the project's 1e-9 m / 1e-9, and it still
# holds for every graph.  Measured on the MI355X: over the five small graphs the largest difference to the restatement's direct solve
# was MEASURED_T / MEASURED_R (robust240's, whose own direct and PCG solves differ by 7.6e-12 m; the others: 1.2e-14 .. 3.8e-13 m), and
# the bound is ten times that.  robust1500, a 6 km ring against scipy's sparse LU: MEASURED_LARGE_T / MEASURED_LARGE_R, where the
# restatement's own sparse-LU and sparse-PCG solves differ by 6.3e-11 m / 6.3e-14 (both 17 steps); ten times the measured translation
# would pass 1e-9, so there 1e-9 itself is the bound, as for the 1 500-node circle of test_pose_graph_gpu.py.
MEASURED_T, MEASURED_R = 7.7e-12, 4.7e-14
MEASURED_LARGE_T, MEASURED_LARGE_R = 3.1e-10, 2.3e-13


@pytest.fixture(scope="module")
def handle():
    m = IcpFastHip(device=0, max_source_points=1024, max_target_points=1024)
    yield m
    m.close()


def _run(handle, g, huber="own", **kw):
    return pose_graph.optimize_robust(handle, g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"],
                                      huber=g["huber"] if isinstance(huber, str) else huber, **kw)


@pytest.mark.parametrize("name", ["robust16", "robust_point"])
def test_stage_parity_of_the_weighted_rows(handle, name):
    """residuals, A, B -- times sqrt(w) where w < 1 -- within 1e-12 relative, the gradient, M^-1 v within 100 eps cond(M): the tolerances of
    pose_graph_gps_cases.check_stage_parity.  Some factor starts above its threshold and some below (the check asserts the first)."""
    g = cases.graph(name)
    _run(handle, g, max_iterations=1)
    n, m = len(g["poses"]), len(g["kinds"])
    v = base.probe_vector(n)
    cases.check_stage_parity(g, pose_graph.last(handle, n, m, v), v)


@pytest.mark.parametrize("name", cases.ALL)
def test_result_and_report_parity(handle, name):
    g, want, st, rep = cases.reference(name)
    poses, stats = _run(handle, g)
    dt, dr = base.pose_difference(poses, want)
    print(name, "difference", dt, dr, stats, "restatement", st["stop"], st["accepted"], st["rejected"], st["damping"])
    assert dt < 1e-9 and dr < 1e-9
    large = name == "robust1500"
    assert dt <= 10 * (MEASURED_LARGE_T if large else MEASURED_T) and dr <= 10 * (MEASURED_LARGE_R if large else MEASURED_R)
    assert 10 * MEASURED_T < 1e-9 and 10 * MEASURED_R < 1e-9 and 10 * MEASURED_LARGE_R < 1e-9
    base.check_costs(stats, st)
    assert (stats["stop_reason"], stats["accepted_steps"], stats["rejected_steps"], stats["damping"]) == (st["stop"], st["accepted"], st["rejected"], st["damping"])
    assert stats["pcg_cap"] == 12 * gps.non_chain_edges(g) + 64 and 0 < stats["pcg_max_iterations"] < stats["pcg_cap"]
    fx = g["fixed"].astype(bool)
    assert (poses[fx] == g["poses"][fx]).all()
    assert (poses[:, 3] == [0, 0, 0, 1]).all()
    # the report, at the device's own result against the restatement's at its own
    m = len(g["kinds"])
    got = pose_graph.last_robust(handle, m)
    cases.check_report_parity(g, (got["norm"], got["weight"], got["cost"]), rep)
    assert abs(got["cost"].sum() - stats["final_cost"]) <= 1e-12 * stats["final_cost"]
    assert (got["weight"][g["bad"]] < 0.1).all() and (np.delete(got["weight"], g["bad"]) == 1.0).all()
    with pytest.raises(SmhipError):
        pose_graph.last_robust(handle, m - 1)                          # a count other than the last call's is refused
    lin = pose_graph.last(handle, len(g["poses"]), m)                  # the linearisation hook still serves the call, after the report too
    again = pose_graph.last_robust(handle, m)                          # ... and leaves the result where the report reads it
    assert all(again[key].tobytes() == got[key].tobytes() for key in got) and np.isfinite(lin["r"]).all()


def test_after_a_plain_call_every_weight_is_one(handle):
    g = cases.graph("robust64")
    m = len(g["kinds"])
    poses, stats = pose_graph.optimize_factors(handle, g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"])
    got = pose_graph.last_robust(handle, m)
    assert (got["weight"] == 1.0).all()
    assert (got["cost"] == got["norm"] ** 2).all() or np.abs(got["cost"] - got["norm"] ** 2).max() <= 1e-12 * got["cost"].max()
    assert abs(got["cost"].sum() - stats["final_cost"]) <= 1e-12 * stats["final_cost"]
    want, _ = cases.plain("robust64")
    assert max(base.pose_difference(poses, want)) < 1e-9
    s = np.array([np.sqrt(cases.robust.norm2(g, want, k)) for k in range(m)])
    assert np.abs(got["norm"] - s).max() <= 1e-7 and got["norm"][g["bad"][0]] > 1.0      # the wrong edge shows in the norm alone
    d = base.circle_cases()["circle64"]                                                   # the oldest entry is served as well
    pose_graph.optimize(handle, d["poses"], d["edges"], d["Z"], fixed=d["fixed"])
    assert (pose_graph.last_robust(handle, len(d["edges"]))["weight"] == 1.0).all()


def test_thresholds_that_never_act_leave_every_bit(handle):
    d = base.circle_cases()["circle64"]
    data = np.stack([gps.between_data(Z) for Z in d["Z"]])
    m = len(data)
    kinds = np.zeros(m, np.uint8)
    want, sw = pose_graph.optimize_factors(handle, d["poses"], kinds, d["edges"], data, fixed=d["fixed"], sigmas=ref.DEFAULT_SIGMAS)
    lin_want = pose_graph.last(handle, 64, m, base.probe_vector(64))
    for hub in (None, np.zeros(m), np.full(m, 1e30)):
        got, sg = pose_graph.optimize_robust(handle, d["poses"], kinds, d["edges"], data, fixed=d["fixed"], sigmas=ref.DEFAULT_SIGMAS, huber=hub)
        assert got.tobytes() == want.tobytes() and sg == sw
        lin = pose_graph.last(handle, 64, m, base.probe_vector(64))
        assert all(lin[key].tobytes() == lin_want[key].tobytes() for key in lin)
    old, so = pose_graph.optimize(handle, d["poses"], d["edges"], d["Z"], fixed=d["fixed"])
    assert old.tobytes() == want.tobytes() and so == sw


def test_two_robust_calls_give_the_same_bits(handle):
    g = cases.graph("robust64")
    a, sa = _run(handle, g)
    ra = pose_graph.last_robust(handle, len(g["kinds"]))
    _run(handle, cases.graph("robust16"))                              # another graph in between leaves nothing behind
    b, sb = _run(handle, g)
    rb = pose_graph.last_robust(handle, len(g["kinds"]))
    assert a.tobytes() == b.tobytes() and sa == sb and all(ra[key].tobytes() == rb[key].tobytes() for key in ra)


def test_refused_thresholds_leave_the_poses_and_the_handle(handle):
    g = cases.graph("robust16")
    before = np.array(g["poses"]).tobytes()
    for bad in (-1.0, np.nan, np.inf):
        hub = g["huber"].copy()
        hub[-1] = bad
        with pytest.raises(SmhipError, match="Huber threshold"):
            _run(handle, g, huber=hub)
        assert np.array(g["poses"]).tobytes() == before
    poses, stats = _run(handle, g)
    assert stats["stop"] in ("step", "cost")


def test_isam_optimizer_with_loop_closure_huber_on_the_device(tmp_path):
    """the AddDetected sequence of test_pose_graph_robust_cpp.py without the Solver hook: the same assertions, and the poses of its CPU run"""
    import test_pose_graph_robust_cpp as cpp
    g = cases.graph("robust16")
    robust, plain = cpp.run_isam("gpu", tmp_path, g, 1.0), cpp.run_isam("gpu", tmp_path, g, 0.0)
    cpp.check_isam(g, robust, plain)
    assert robust["entries"][2] > 0 and plain["entries"] == [plain["solves"], 0, 0]      # thresholds: the robust entry; none: the oldest one alone
    for dev, huber in ((robust, 1.0), (plain, 0.0)):
        host = cpp.run_isam("host", tmp_path, g, huber)
        dt, dr = base.pose_difference(dev["poses"], host["poses"])
        print("loop_closure_huber", huber, "device against the CPU run", dt, dr)
        assert dt < 1e-9 and dr < 1e-9
        assert [(t, s) for t, s, _, _ in dev["report"]] == [(t, s) for t, s, _, _ in host["report"]]
        assert all(abs(a[2] - b[2]) <= 1e-7 and (a[3] == b[3] == 1.0 or abs(a[3] - b[3]) <= 1e-7 * b[3]) for a, b in zip(dev["report"], host["report"]))
