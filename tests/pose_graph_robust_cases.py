"""Graphs with a wrong loop edge (or a wrong ENU fix) and Huber thresholds, shared by the CPU, C++ and device tests, all against
tests/pose_graph_robust_ref.py.  A ring case is pose_graph_ref.circle_drive(n, seed=1) with its three good loops plus one corrupted
loop (3, 3 + n - 4) measured as truth_a^-1 truth_b make_pose((0, 0, yaw), offset), without noise; the threshold is 1 on the four loop
edges and 0 on the chain.  The restatement's results are computed once per process and left unchanged.  No seed had to change: the
conditions tests/test_pose_graph_robust_ref.py asserts hold with seed 1 at every size."""
import functools

import numpy as np

import pose_graph_cases as base
import pose_graph_gps_cases as gps_cases
import pose_graph_gps_ref as gps
import pose_graph_ref as ref
import pose_graph_robust_ref as robust

RINGS = {"robust16": (16, (3.0, 0.0, 0.0), 0.0), "robust64": (64, (3.0, 0.0, 0.0), 0.0), "robust65": (65, (3.0, 0.0, 0.0), 0.1),
         "robust240": (240, (3.0, 1.0, 0.0), 0.1)}
SMALL = tuple(RINGS) + ("robust_point",)
ALL = SMALL + ("robust1500",)


def as_factors(drive, n_good_loops, bad, k=1.0):
    """A drive of pose_graph_ref as a factor graph: its BETWEEN factors, then the corrupted loops `bad`, [(a, b, offset, yaw)]; the
    threshold k on every loop edge, good or bad, 0 on the chain.  g["bad"]: the corrupted factors' indices, g["loops"]: all loop factors'."""
    n = len(drive["poses"])
    factors = [(gps.BETWEEN, int(i), int(j), gps.between_data(Z), ref.DEFAULT_SIGMAS) for (i, j), Z in zip(drive["edges"], drive["Z"])]
    first_bad = len(factors)
    for a, b, offset, yaw in bad:
        Z = ref.inv(drive["truth"][a]) @ drive["truth"][b] @ ref.make_pose((0.0, 0.0, yaw), offset)
        factors.append((gps.BETWEEN, a, b, gps.between_data(Z), ref.DEFAULT_SIGMAS))
    g = gps.make_graph(drive["poses"], drive["fixed"], factors)
    hub = np.zeros(len(factors))
    hub[n - 1:] = k                                   # the chain is factors 0 .. n - 2
    assert first_bad == n - 1 + n_good_loops
    g.update(huber=hub, truth=drive["truth"], bad=list(range(first_bad, len(factors))), loops=list(range(n - 1, len(factors))))
    return g


def ring(n, offset, yaw):
    return as_factors(ref.circle_drive(n, seed=1), 3, [(3, 3 + n - 4, offset, yaw)])


def point_case():
    """pose_graph_gps_cases' chain of 23 nodes with a fix on each, the fix of node 11 moved 5 m east; the threshold 1 on every POINT"""
    src = gps_cases.graph("chain23_all")
    g = {key: (np.array(val) if isinstance(val, np.ndarray) else val) for key, val in src.items()}
    points = np.flatnonzero(g["kinds"] == gps.POINT)
    bad = int(points[11])
    assert g["ij"][bad][1] == 11
    g["data"][bad, 3] += 5.0
    hub = np.zeros(len(g["kinds"]))
    hub[points] = 1.0
    g.update(huber=hub, bad=[bad], loops=[int(p) for p in points])
    return g


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in RINGS:
        return ring(*RINGS[name])
    if name == "robust_point":
        return point_case()
    if name == "robust1500":
        # pose_graph_cases.large_circle's drive plus two corrupted loops that contradict each other, 3 m ahead and 3 m behind.  (Two
        # that agree -- both 3 m ahead -- are a second hypothesis held by two edges against six: the nearest good loop then ends at
        # weight 0.36 and the restatement itself runs into max_iterations, 26 accepted and 24 rejected steps.  That is the method,
        # not a case to test an implementation on.  With (-3, 1, 0) for the second the restatement stops a step after a decrease of
        # 1.006 bands, which another summation order could have taken for the stop; with (-3, -1, 0) its last three decreases are
        # 11.5, 2.4 and 0.52 bands.)
        n = 1500
        d = ref.circle_drive(n, seed=3, loops=[(k, None) for k in range(6)], overlap=8)
        return as_factors(d, 6, [(6, 6 + n - 8, (3.0, 0.0, 0.0), 0.0), (7, 7 + n - 8, (-3.0, -1.0, 0.0), 0.1)])
    raise KeyError(name)


def default_solver(name):
    return "sparse" if name == "robust1500" else "direct"


@functools.lru_cache(maxsize=None)
def reference(name, solver=None):
    """(graph, the restatement's poses, its stats, its report at those poses) -- computed once"""
    g = graph(name)
    poses, st = robust.optimize(g, solver=solver or default_solver(name))
    poses.setflags(write=False)
    return g, poses, st, robust.report(g, poses)


@functools.lru_cache(maxsize=None)
def plain(name):
    """the same graph solved without thresholds by pose_graph_gps_ref.optimize: (poses, stats)"""
    poses, st = gps.optimize(graph(name), solver=default_solver(name))
    poses.setflags(write=False)
    return poses, st


def truth_error(g, poses):
    """the largest distance of a node from the truth, in m (the frame node of a GPS graph left out)"""
    n = len(g["truth"])
    return float(np.linalg.norm(poses[:n, :3, 3] - g["truth"][:, :3, 3], axis=1).max())


def error(name, g, poses):
    """What a wrong edge costs.  A ring: the largest distance from the truth.  robust_point: the largest distance of the antenna
    positions, mapped by the frame node, from the truth's ENU positions -- its chain starts 0.1 m / rad off the truth with only node 0
    held, so the map frame is not the truth's and the clean graph itself ends 1.95 m from it, with or without the wrong fix."""
    return gps_cases.enu_error(g, poses) if name == "robust_point" else truth_error(g, poses)


def check_stage_parity(g, got, v):
    """pose_graph_gps_cases.check_stage_parity at the same tolerances, on the weighted rows, plus the weights: exactly 1 where the
    restatement's is 1, within 1e-12 relative elsewhere (one square root and one division of s_f^2, itself a sum of six squares of
    numbers that agree to 1e-12)."""
    r, A, B, w = robust.linearize(g, g["poses"])
    for name, want, have in (("r", r, got["r"]), ("A", A, got["A"]), ("B", B, got["B"])):
        err = np.abs(have - want) / np.maximum(1.0, np.abs(want))
        print(name, "worst relative difference", err.max() if err.size else 0.0)
        assert (err <= 1e-12).all(), (name, err.max())
    if "w" in got:
        one = w == 1.0
        print("weights below 1:", int((~one).sum()), "worst relative difference", np.abs(got["w"][~one] / w[~one] - 1.0).max() if (~one).any() else 0.0)
        assert (~one).any() and (got["w"][one] == 1.0).all() and (np.abs(got["w"][~one] - w[~one]) <= 1e-12 * w[~one]).all()
    pt, pr = g["kinds"] == gps.POINT, g["kinds"] == gps.PRIOR
    assert (got["r"][pt, 3:] == 0.0).all() and (got["A"][pt, 3:] == 0.0).all() and (got["B"][pt, 3:] == 0.0).all()
    assert (got["B"][pr] == 0.0).all()
    n = len(g["poses"])
    H, grad = robust.assemble(g, g["poses"])
    scale = max(np.abs(A).max() * np.abs(r).max() * 6 * 4, 1.0)
    deg = np.bincount(np.concatenate([g["ij"][:, 0], g["ij"][~pr, 1]]), minlength=n).max()
    print("g worst difference", np.abs(got["g"].ravel() - grad).max(), "scale", scale, "largest degree", deg)
    assert np.abs(got["g"].ravel() - grad).max() <= 1e-12 * scale * max(1.0, deg / 4.0)
    M = ref.chain_part(H)
    fx = np.repeat(np.asarray(g["fixed"]).astype(bool), 6)
    vv = np.where(fx, 0.0, v.ravel())
    want = np.linalg.solve(M, vv)
    cond = np.linalg.cond(M)
    have = got["minv_v"].ravel()
    print("M^-1 v worst difference", np.abs(have - want).max(), "bound", 100 * base.EPS * cond * np.abs(want).max(), "cond", cond)
    assert np.abs(have - want).max() <= 100 * base.EPS * cond * np.abs(want).max()
    back = np.abs(M @ have - vv)
    assert (back <= 1e-12 * (np.abs(M) @ np.abs(have) + np.abs(vv))).all(), back.max()
    assert (have[fx] == 0.0).all()


def check_report_parity(g, got, want):
    """got, want: (norm, weight, cost term).  norm within 1e-7 absolute: poses within 1e-9 m / 1e-9, sigma at least 0.1, twelve
    whitened-row entries over two poses, so |ds| <= 12 x 1e-9 / 0.1 ~ 1.2e-7 in the worst direction and far less in fact.  Weights
    that are 1 in the restatement are exactly 1; the others (k / s with s above k) within 1e-7 relative."""
    (s, w, c), (ws, ww, wc) = got, want
    print("report: norm worst difference", np.abs(s - ws).max(), "weights below 1", int((ww < 1.0).sum()))
    assert (np.abs(s - ws) <= 1e-7).all()
    one = ww == 1.0
    assert (w[one] == 1.0).all()
    assert (np.abs(w[~one] - ww[~one]) <= 1e-7 * ww[~one]).all()
    # the term: d(s^2) = 2 s ds and d(2 k s - k^2) = 2 k ds with ds <= 1e-7 and k = 1: below 1e-6 max(1, term) at every s
    assert (np.abs(c - wc) <= 1e-6 * np.maximum(1.0, np.abs(wc))).all()
