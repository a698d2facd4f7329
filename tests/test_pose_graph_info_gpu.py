"""The device pose-graph optimiser with full square-root informations (smhip_pose_graph_optimize_info, one kernel launch per call) on
the graphs of tests/pose_graph_info_cases.py: the first linearisation through smhip_pose_graph_last, the result against the same
loop's run on the CPU (tests/cpp/test_pose_graph_info.cc, HostCtx) at test_pose_graph_calib_gpu.py's tolerance, the case that shows
the point, the bits of the *_calib entry when no factor carries an L, and the refusals."""
import numpy as np
import pytest

import pose_graph_calib_cases as calib_cases
import pose_graph_cases as base
import pose_graph_info_cases as cases
import pose_graph_info_ref as pgi
import pose_graph_robust_cases as robust_cases
import test_pose_graph_info_cpp as cpp
from staticmapping_amd import IcpFastHip, SmhipError, pose_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    m = IcpFastHip(device=0, max_source_points=1024, max_target_points=1024)
    yield m
    m.close()


def _run(handle, g, **kw):
    a = {**dict(huber=g.get("huber"), sqrt_information=g["L"]), **kw}
    return pose_graph.optimize_info(handle, g["poses"], g["kinds"], g["ij"], g["data"], fixed=g["fixed"], sigmas=g["sigmas"], **a)


@pytest.mark.parametrize("name", cases.NAMES)
def test_the_device_follows_the_cpu_run_and_the_restatement(handle, name, tmp_path):
    """The bound of a graph is ten times the restatement's own direct-against-PCG disagreement on it (where the two agree to the bit,
    the rounding of the largest coordinate, 1e-15 |t|), as in test_pose_graph_calib_gpu.py."""
    g, want, st = cases.reference(name)
    _, other, _ = cases.reference(name, "pcg")
    own = max(base.pose_difference(want, other))
    floor = 1e-15 * np.abs(want[:, :3, 3]).max()
    n, m = len(g["poses"]), len(g["kinds"])
    v = base.probe_vector(n)
    _run(handle, g, max_iterations=1)
    cases.check_stage_parity(g, pose_graph.last(handle, n, m, v))
    host, host_stats, _, _, _ = cpp.host_solve(g, tmp_path, v)
    poses, stats = _run(handle, g)
    dt, dr = base.pose_difference(poses, host)
    rt, rr = base.pose_difference(poses, want)
    print(name, "device against the CPU run", dt, dr, "against the restatement", rt, rr, "restatement's direct against PCG", own, "bound", 10 * max(own, floor), stats)
    assert max(dt, dr) <= 10 * max(own, floor) and max(rt, rr) <= 10 * max(own, floor)
    base.check_costs(stats, st)
    assert (stats["stop_reason"], stats["accepted_steps"], stats["rejected_steps"], stats["damping"]) == \
        (host_stats["stop_reason"], host_stats["accepted_steps"], host_stats["rejected_steps"], host_stats["damping"]) == (st["stop"], st["accepted"], st["rejected"], st["damping"])
    fx = np.asarray(g["fixed"]).astype(bool)
    assert (poses[fx] == g["poses"][fx]).all() and (poses[:, 3] == [0, 0, 0, 1]).all()
    rep = pose_graph.last_robust(handle, m)                               # the report serves the new entry
    robust_cases.check_report_parity(g, (rep["norm"], rep["weight"], rep["cost"]), pgi.report(g, want))


def test_edges_that_do_not_see_x_let_the_points_decide_it(handle):
    plain, _ = _run(handle, cases.graph("chain6_sigma"))
    weak, _ = _run(handle, cases.graph("chain6_weak_x"))
    print("distance from the POINT targets along x: sigma edges", cases.x_miss(plain), "weak-x edges", cases.x_miss(weak))
    assert cases.x_miss(weak).max() < 0.05 and cases.x_miss(plain).max() > 0.05


def test_two_calls_give_the_same_bits(handle):
    g = cases.graph("ring16_full")
    a, sa = _run(handle, g)
    _run(handle, cases.graph("chain6_weak_x"))                            # another graph in between leaves nothing behind
    b, sb = _run(handle, g)
    assert a.tobytes() == b.tobytes() and sa == sb


@pytest.mark.parametrize("name", ["ring16_free", "gps24_free"])
def test_without_an_information_the_bytes_are_the_calib_entrys(handle, name):
    g = calib_cases.graph(name)
    n, m = len(g["poses"]), len(g["kinds"])
    args = (handle, g["poses"], g["kinds"], g["ij"], g["data"])
    kw = dict(fixed=g["fixed"], sigmas=g["sigmas"], huber=g["huber"])
    want, sw = pose_graph.optimize_calib(*args, **kw)
    lw = pose_graph.last(handle, n, m, base.probe_vector(n))
    rw = pose_graph.last_robust(handle, m)
    _run(handle, cases.graph("ring16_full"))                              # a call with informations in between leaves nothing behind
    for extra in (dict(), dict(info_index=np.full(m, -1, np.int32), sqrt_info=np.zeros((1, 36))), dict(sqrt_information=[None] * m)):
        got, sg = pose_graph.optimize_info(*args, **kw, **extra)
        lg = pose_graph.last(handle, n, m, base.probe_vector(n))
        rg = pose_graph.last_robust(handle, m)
        assert got.tobytes() == want.tobytes() and sg == sw
        assert all(lg[key].tobytes() == lw[key].tobytes() for key in lw) and all(rg[key].tobytes() == rw[key].tobytes() for key in rw)


def test_refused_calls_leave_the_poses_and_the_handle(handle):
    g = cases.graph("ring16_full")
    index, rows = cases.abi_arrays(g)
    before = np.array(g["poses"]).tobytes()
    be = int(np.flatnonzero(index >= 0)[0])
    bad_index = index.copy()
    bad_index[be] = len(index)
    nan_rows = rows.copy()
    nan_rows[index[be], 7] = np.nan
    flat_rows = rows.copy()
    flat_rows[index[be]] = 0.0
    on_prior = index.copy()
    on_prior[int(np.flatnonzero(g["kinds"] == pose_graph.PRIOR)[0])] = 0
    for match, change in (("index out of range", dict(info_index=bad_index)), ("not finite", dict(sqrt_info=nan_rows)), ("is singular", dict(sqrt_info=flat_rows)),
                          ("is no BETWEEN", dict(info_index=on_prior))):
        a = {**dict(info_index=index, sqrt_info=rows), **change}
        with pytest.raises(SmhipError, match=match):
            _run(handle, g, sqrt_information=None, **a)
        assert np.array(g["poses"]).tobytes() == before
    poses, stats = _run(handle, g)
    assert stats["stop"] in ("step", "cost")


def test_a_corridor_end_to_end(tmp_path):
    """Three 2 000-point one-frame submaps in a corridor along x, 1 m apart, whose chain guesses say 0.7 m (the fixture and why it has
    this shape: tests/cpp/test_pose_graph_info.cc, CorridorCloud).  builder::ConnectSubmaps and CloseLoop measure every accepted
    match's information, IsamOptimizer takes it with use_edge_information and an odometer on every frame (1 m along the corridor:
    right; 0.3 m per frame across: wrong).

    Where the bounds come from.  No normal has an x component (asserted: below 1e-6), so the x translation is the direction the
    clouds do not see: it must be every edge's `weakest` (|cos| > 0.99) with a strength below 1e-2, which inflates the edge's x sigma
    past the odometer's 1.5 m; every other direction is pinned (strength above 10: the floor's sigma to within a tenth).  With the
    strength at 0 the edges' x sigma is max_inflation x 0.15 = 15 m against the odometer's 1.5 m: a node's x is the weighted mean of
    the odometer's k and the chain's 0.7 k with weights 1 / 1.5^2 and at most 3 / 15^2 (three edges), so it ends within
    0.6 x 0.0133 / 0.458 = 0.02 m of the odometer; 0.05 m is asserted.  With the fixed sigmas the weights are 1 / 1.5^2 against
    1 / 0.15^2 and x stays within 0.01 x 0.6 = 0.006 m ... 0.2 m of the chain's 0.7 k (asserted as before).  Across the corridor the
    edges keep 0.15 m against the odometer's 1.5 m either way: y ends within 0.01 x 0.6 m of the scan matches' 0; 0.15 m, the scan
    matches' sigma, is asserted.  With the option off the poses are today's, and measuring without using changes no bit."""
    import json
    import subprocess
    out = subprocess.run([cpp._build_exe(), "corridor"], text=True, capture_output=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    on, off, plain = (np.array(res[k]).reshape(3, 4, 4) for k in ("on", "measured_but_off", "plain"))
    print("x with the informations", on[:, 0, 3], "without", plain[:, 0, 3], "y with", on[:, 1, 3], "without", plain[:, 1, 3], "kept", res["kept"],
          "worst |n_x|", res["worst_normal_x"])
    assert off.tobytes() == plain.tobytes()
    assert res["worst_normal_x"][0] < 1e-6                                 # the fixture's property: no estimated normal sees x
    for edge in ("chain0", "chain1", "loop"):
        h, w = np.array(res[edge + "_strength"]), np.array(res[edge + "_weakest"])
        print(edge, "strength", h, "weakest", w)
        assert abs(w[3]) > 0.99 and h[0] < 1e-2 and h[1] > 10.0
    assert min(res["kept"]) > 6
    k = np.arange(3)
    assert np.abs(on[:, 0, 3] - 1.0 * k).max() <= 0.05                     # along: the odometer's 1 m steps
    assert np.abs(on[:, 1, 3]).max() <= 0.15                               # across: the scan matches' 0, not the odometer's 0.3 m steps
    assert np.abs(plain[:, 0, 3] - 0.7 * k).max() <= 0.2 and np.abs(plain[:, 1, 3]).max() <= 0.15
    assert np.abs(plain[1:, 0, 3] - 1.0 * k[1:]).min() > 0.2               # ... which is not where the odometer is
