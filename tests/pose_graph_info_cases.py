"""Graphs whose BETWEEN factors carry a full 6x6 square-root information, shared by the CPU, C++ and device tests, all against
tests/pose_graph_info_ref.py.  The restatement's results are computed once per process and left unchanged.

  chain6_sigma / chain6_weak_x   the case that shows the point: six nodes 1 m apart along x, node 0 fixed, a chain of BETWEENs, and on
                                 every free node a POINT factor (sigma 0.15 m, frame node 0) whose target lies 0.5 m further along x.
                                 _sigma: the chain edges claim 0.15 m on every axis and the nodes end between the two.  _weak_x: the
                                 edges carry the L of an alignment that does not see x (tests/icp_information_ref.edge_information of
                                 a rank-5 H): 15 m along x, the floor elsewhere -- the nodes follow the POINT targets along x
  ring16_diag                    pose_graph_calib_cases' ring16_free with L = diag(1 / sigma) on every BETWEEN: the sigma form's poses
  ring16_full                    the same ring with the L of a random alignment on every BETWEEN (dense, no two alike), HANDEYE
                                 factors under Huber beside them
"""
import functools

import numpy as np

import icp_information_ref as info
import pose_graph_calib_cases as calib_cases
import pose_graph_calib_ref as calib
import pose_graph_gps_ref as gps
import pose_graph_info_ref as pgi
import pose_graph_ref as ref

PULL = 0.5
NAMES = ("chain6_sigma", "chain6_weak_x", "ring16_diag", "ring16_full")


def weak_x_information():
    """the edge of an alignment that sees everything but the translation along x"""
    H = np.diag([4.0e4, 4.0e4, 4.0e4, 0.0, 2.0e3, 2.0e3])
    return info.edge_information(H, sum_r2=0.02 ** 2 * 994, kept=1000)["L"]


def chain6(weak):
    n = 6
    poses = np.stack([ref.make_pose((0.0, 0.0, 0.0), (float(k), 0.0, 0.0)) for k in range(n)])
    step = ref.make_pose((0.0, 0.0, 0.0), (1.0, 0.0, 0.0))
    factors = [(calib.BETWEEN, k, k + 1, gps.between_data(step), ref.DEFAULT_SIGMAS, 0.0) for k in range(n - 1)]
    factors += [(calib.POINT, 0, k, gps.point_data(np.zeros(3), np.array([k + PULL, 0.0, 0.0])), gps.GPS_SIGMAS, 0.0) for k in range(1, n)]
    g = calib.make_graph(list(poses), [1] + [0] * (n - 1), factors)
    L = [weak_x_information() if weak and k < n - 1 else None for k in range(len(factors))]
    return pgi.with_information(g, L)


def random_information(rng):
    """the edge of a made-up alignment: 200 rows J = [s x m ; m] of points a few metres out"""
    s = rng.uniform(-8.0, 8.0, size=(200, 3))
    m = rng.normal(size=(200, 3))
    m /= np.linalg.norm(m, axis=1, keepdims=True)
    J = np.concatenate([np.cross(s, m), m], axis=1)
    # (the scale puts the whitened eigenvalues h around 1, where neither the floor nor the alignment alone decides the edge)
    return info.edge_information(J.T @ J, sum_r2=rng.uniform(0.02, 0.2), kept=200, information_scale=3.0e-5)["L"]


def ring16(full):
    g = calib_cases.graph("ring16_free")
    rng = np.random.default_rng(16)
    L = []
    for k in range(len(g["kinds"])):
        if g["kinds"][k] != calib.BETWEEN:
            L.append(None)
        else:
            L.append(random_information(rng) if full else np.diag(1.0 / g["sigmas"][k]))
    return pgi.with_information(g, L)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name.startswith("chain6"):
        return chain6(name == "chain6_weak_x")
    return ring16(name == "ring16_full")


@functools.lru_cache(maxsize=None)
def reference(name, solver="direct"):
    """(graph, the restatement's poses, its stats) -- computed once"""
    g = graph(name)
    poses, st = pgi.optimize(g, solver=solver)
    poses.setflags(write=False)
    return g, poses, st


def abi_arrays(g):
    """(info_index [F] int32, sqrt_info [K, 36]) of the graph's L"""
    index = np.full(len(g["kinds"]), -1, np.int32)
    rows = []
    for k, L in enumerate(g["L"]):
        if L is not None:
            index[k] = len(rows)
            rows.append(L.reshape(36))
    return index, (np.stack(rows) if rows else np.zeros((0, 36)))


def check_stage_parity(g, got):
    """the first linearisation: residuals, A, B within 1e-12 relative of the restatement's (a row of L times a column is six more
    products on top of pose_graph_cases.check_stage_parity's count, of numbers up to max(1, the entry)); the gradient as there"""
    r, A, B, _ = pgi.linearize(g, g["poses"])
    for name, want, have in (("r", r, got["r"]), ("A", A, got["A"]), ("B", B, got["B"])):
        err = np.abs(have - want) / np.maximum(1.0, np.abs(want))
        print(name, "worst relative difference", err.max())
        assert (err <= 1e-12).all(), (name, err.max())
    _, grad = pgi.assemble(g, g["poses"])
    pr = g["kinds"] == calib.PRIOR
    deg = np.bincount(np.concatenate([g["ij"][:, 0], g["ij"][~pr, 1]]), minlength=len(g["poses"])).max()
    scale = max(np.abs(A).max() * np.abs(r).max() * 6 * 4, 1.0)
    assert np.abs(got["g"].ravel() - grad).max() <= 1e-12 * scale * max(1.0, deg / 4.0)


def x_miss(poses):
    """the chain6 nodes' distance from their POINT targets along x, in m"""
    return np.abs(np.asarray(poses)[1:6, 0, 3] - (np.arange(1, 6) + PULL))
