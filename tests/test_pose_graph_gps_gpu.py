"""The device pose-graph optimiser with PRIOR and POINT factors (smhip_pose_graph_optimize_factors, one kernel launch per call)
against tests/pose_graph_gps_ref.py: stage by stage through smhip_pose_graph_last, the result against the restatement's direct
solve, bits, refusals and the iteration counts.  The graphs are those of tests/pose_graph_gps_cases.py: chains of 1, 2, 4, 23, 62, 63
and 64 nodes plus the frame node (63 / 64 / 65 nodes in all straddle a level of the cyclic reduction; the frame node is adjacent to
the last chain node, so one POINT lands in a chain block) with a factor on every node, on every second node and on the last node
only; the 25 + 1 alone graph, which has no chain edge at all; and one drive of 1 100 nodes with a factor on each."""
import numpy as np
import pytest

import pose_graph_cases as base
import pose_graph_gps_cases as cases
import pose_graph_gps_ref as gps
import pose_graph_ref as ref
from staticmapping_amd import IcpFastHip, SmhipError, pose_graph

pytestmark = pytest.mark.gpu

# Result parity, in metres and in rotation-matrix entries.  Measured on the MI355X over every graph below: the largest difference to
# the restatement's direct solve was MEASURED_T / MEASURED_R; the bound is ten times that.  A measured value above ten times the
# restatement's own direct-against-PCG disagreement on the same graph fails outright: that would be a finding, not a tolerance.
# (Both largest values are the alone graph's, whose start is 370 m and 0.4 rad from its end and whose own two solves differ by
# 3.4e-12; the chains differ by at most 1.1e-12 m / 1.3e-14.  Where the restatement's two solves agree to the bit -- one iteration
# each, chains of 1, 2 and 4 nodes -- the floor is the rounding of the largest coordinate, 1e-15 |t|: a few ulp.)
MEASURED_T, MEASURED_R = 3.4e-12, 2.2e-14
BOUND_T, BOUND_R = 10 * MEASURED_T, 10 * MEASURED_R
MEASURED_LARGE_T, MEASURED_LARGE_R = 5.2e-11, 1.1e-12  # the drive of 1 100 nodes: what its own direct and PCG solves differ by (5.1e-11)
GRAPHS = sorted(cases.chain_cases()) + ["alone"]


@pytest.fixture(scope="module")
def handle():
    m = IcpFastHip(device=0, max_source_points=1024, max_target_points=1024)
    yield m
    m.close()


def _run(handle, g, **kw):
    return pose_graph.optimize_factors(handle, g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"], **kw)


@pytest.mark.parametrize("name", GRAPHS)
def test_stage_parity_through_the_last_hook(handle, name):
    """residuals, A, B within 1e-12 relative, rows 3-5 of a POINT exactly zero, the gradient, M^-1 v within 100 eps cond(M)"""
    g = cases.graph(name)
    _run(handle, g, max_iterations=1)
    n, m = len(g["poses"]), len(g["kinds"])
    v = base.probe_vector(n)
    cases.check_stage_parity(g, pose_graph.last(handle, n, m, v), v)


@pytest.mark.parametrize("name", GRAPHS)
def test_result_parity_with_the_direct_solve(handle, name):
    g, want, st = cases.reference(name)
    same, own = cases.qualifies(name)
    assert same and own < 1e-10 and cases.gradient_ratio(g, want) < 1e-9   # the graph qualifies for device parity
    poses, stats = _run(handle, g, max_iterations=100 if name == "alone" else 50)
    dt, dr = base.pose_difference(poses, want)
    ratio = cases.gradient_ratio(g, poses)
    print(name, "difference", dt, dr, "restatement's direct against PCG", own, "gradient ratio", ratio, stats, "restatement", st["stop"], st["accepted"], st["rejected"])
    assert max(dt, dr) <= 10 * max(own, 1e-15 * np.abs(want[:, :3, 3]).max())    # (a disagreement of exactly 0 -- both solves exact in one iteration -- leaves the rounding of one entry)
    assert dt <= BOUND_T and dr <= BOUND_R
    assert ratio < 1e-9
    base.check_costs(stats, st)
    assert (stats["accepted_steps"], stats["rejected_steps"], stats["damping"]) == (st["accepted"], st["rejected"], st["damping"])
    assert stats["stop_reason"] == st["stop"]
    assert stats["pcg_cap"] == 12 * gps.non_chain_edges(g) + 64 and 0 < stats["pcg_max_iterations"] < 30
    assert stats["levels"] == int(np.ceil(np.log2(len(g["poses"]))))
    fx = g["fixed"].astype(bool)
    assert (poses[fx] == g["poses"][fx]).all()
    assert (poses[:, 3] == [0, 0, 0, 1]).all()


def test_more_factors_than_threads(handle):
    """1 100 nodes, 2 200 factors on 1 024 threads, a frame node of degree 1 101: against the restatement's sparse direct solve, which
    its own sparse PCG solve follows within 1e-10 with the same counts (the qualification).  MEASURED_LARGE_*: as above."""
    g, want, st = cases.large_drive()
    same, own, own_pcg = st["own"]
    assert same and own < 1e-10 and cases.gradient_ratio(g, want) < 1e-9
    poses, stats = _run(handle, g)
    dt, dr = base.pose_difference(poses, want)
    ratio = cases.gradient_ratio(g, poses)
    before, after = cases.enu_error(g, g["poses"]), cases.enu_error(g, poses)
    print("difference", dt, dr, "restatement's direct against PCG", own, "its longest solve", own_pcg, "gradient ratio", ratio, stats, "restatement", st["stop"], st["accepted"],
          st["rejected"], "ENU-frame error before", before, "after", after)
    assert max(dt, dr) <= 10 * own
    assert dt <= 10 * MEASURED_LARGE_T and dr <= 10 * MEASURED_LARGE_R
    assert ratio < 1e-9
    base.check_costs(stats, st)
    assert (stats["accepted_steps"], stats["rejected_steps"], stats["damping"]) == (st["accepted"], st["rejected"], st["damping"])
    assert 0 < stats["pcg_max_iterations"] < 30
    assert after < 0.1 * before
    lin = pose_graph.last(handle, len(g["poses"]), len(g["kinds"]))
    r, A, B = gps.linearize(g, g["poses"])
    for have, wanted in ((lin["r"], r), (lin["A"], A), (lin["B"], B)):
        assert (np.abs(have - wanted) <= 1e-12 * np.maximum(1.0, np.abs(wanted))).all()
    with pytest.raises(SmhipError):
        pose_graph.last(handle, len(g["poses"]), len(g["kinds"]) - 1)  # sizes other than the last call's are refused


def test_two_calls_give_the_same_bits(handle):
    g = cases.graph("chain64_all")
    a, sa = _run(handle, g)
    _run(handle, cases.graph("chain23_second"))                        # another graph in between leaves nothing behind
    b, sb = _run(handle, g)
    assert a.tobytes() == b.tobytes() and sa == sb


def test_null_kinds_give_the_bits_of_the_old_call(handle):
    g, _, _ = base.reference("n65")
    old, so = pose_graph.optimize(handle, g["poses"], g["edges"], g["Z"], fixed=g["fixed"])
    data = np.stack([gps.between_data(Z) for Z in g["Z"]])
    new, sn = pose_graph.optimize_factors(handle, g["poses"], None, g["edges"], data, fixed=g["fixed"])
    assert old.tobytes() == new.tobytes() and so == sn
    lin = pose_graph.last(handle, len(g["poses"]), len(g["edges"]))    # the hook serves whichever call ran last
    assert np.abs(lin["r"]).max() > 0.0
    zeros, sz = pose_graph.optimize_factors(handle, g["poses"], np.zeros(len(data), np.uint8), g["edges"], data, fixed=g["fixed"], sigmas=ref.DEFAULT_SIGMAS)
    assert old.tobytes() == zeros.tobytes() and so == sz


def test_refused_calls_leave_the_poses_untouched(handle):
    g = cases.graph("chain4_all")

    def refused(**change):
        a = {**g, **change}
        before = np.array(a["poses"]).tobytes()
        with pytest.raises(SmhipError):
            pose_graph.optimize_factors(handle, a["poses"], a["kinds"], a["ij"], a["data"], fixed=a["fixed"], sigmas=a["sigmas"])
        assert np.array(a["poses"]).tobytes() == before
    k = g["kinds"].copy()
    k[0] = 7
    refused(kinds=k)
    prior = int(np.flatnonzero(g["kinds"] == gps.PRIOR)[0])
    point = int(np.flatnonzero(g["kinds"] == gps.POINT)[0])
    e = g["ij"].copy()
    e[prior] = (4, 3)
    refused(ij=e)
    d = g["data"].copy()
    d[point, 4] = np.nan
    refused(data=d)
    refused(sigmas=None)
    keep = np.flatnonzero(g["kinds"] != gps.PRIOR)                     # the frame node with POINT factors only
    refused(kinds=g["kinds"][keep], ij=g["ij"][keep], data=g["data"][keep], sigmas=g["sigmas"][keep])
    poses, stats = _run(handle, g)                                     # and the handle still works
    assert stats["stop"] in ("step", "cost")


def test_a_chain_held_by_two_points_alone_ends_as_numeric(handle):
    """passes the plan -- every free node has a BETWEEN, the component has the frame's PRIOR -- but two POINT factors leave the chain
    a rotation about the line through them: M is singular, the kernel says so and the poses stay as given"""
    d = base.chain_graph(4, 5)
    enu = cases.enu_of(d["truth"], 5)
    g = gps.with_gps(d, enu, np.zeros(3), np.eye(4), [0, 3])
    g["fixed"] = np.zeros(5, np.uint8)
    before = g["poses"].tobytes()
    with pytest.raises(SmhipError, match="pivot"):
        _run(handle, g)
    assert g["poses"].tobytes() == before


def test_isam_optimizer_bounds_the_drift_of_a_drive_that_never_returns(tmp_path):
    """40 submaps on three quarters of a circle, a fix on each; the second half is fed with 0.5 m and 0.5 degrees of drift.  There is no
    loop candidate, so no clouds are needed.  The factor count is the restated rule's, GetGpsCoordTransform() ends within the
    alone-solve test's 0.30 m / 0.014 rad of the truth, and the antenna positions in the ENU frame are closer to the truth than the
    fed poses are even when those are mapped by the true frame."""
    import test_pose_graph_gps_cpp as cpp
    truth, fed = cpp.quarter_drive(drift_from=20)
    enu = cases.enu_of(truth, 11)
    has = [True] * len(fed)
    code, res = cpp.run_isam("gpu", tmp_path, fed, enu, has)
    assert code == 0 and res["ok"], res
    want = cpp.check_against_the_rule(res, has)
    assert want["trigger"] == 25 and res["gps_factors"] == 39 and res["nodes"] == 41
    assert res["stop_reason"] in (1, 2) and res["alone_stop_reason"] in (1, 2) and res["alone_rejected"] == 0
    assert 0 < res["pcg_max_iterations"] < 30 and 0 < res["alone_pcg_max"] < 30
    G = np.array(res["gps_coord"]).reshape(4, 4)
    poses = np.array(res["poses"]).reshape(len(fed), 4, 4)
    dt, dr = np.linalg.norm(G[:3, 3] - cases.G[:3, 3]), np.linalg.norm(ref.log_so3(cases.G[:3, :3].T @ G[:3, :3]))
    truth_enu = cases.enu_positions(truth, cases.G)
    before = np.linalg.norm(cases.enu_positions(fed, cases.G) - truth_enu, axis=1).max()
    after = np.linalg.norm(cases.enu_positions(poses, G) - truth_enu, axis=1).max()
    print("frame off by %.3f m, %.4f rad; ENU-frame error %.3f m before, %.3f m after; alone solve: %d steps, pcg max %d; last solve pcg max %d"
          % (dt, dr, before, after, res["alone_accepted"], res["alone_pcg_max"], res["pcg_max_iterations"]))
    assert dt < 0.30 and dr < 0.014
    assert before > 0.45 and after < before
    assert np.abs(poses[0] - truth[0]).max() == 0.0                     # the first submap is the gauge
