"""The graph a join of two maps is solved on (include/smhip/multi_trajectory.h: MultiTrajectoryOptimizer as MultiTrajectoryMapBuilder
feeds it), restated in numpy, f64, over tests/pose_graph_robust_ref.py, which is imported as it is and does every solve.

  nodes       the base map's submaps, then the incremental map's: a submap's node is its place in that concatenation.
  factors     in the order PoseGraph::FlattenFactors emits them: the BETWEEN factors as they were added -- the base map's connections
              (k, k + 1); then, submap by submap of the incremental map, the loop constraints whose source it is; then the
              incremental map's connections -- and after them the PRIORs: one on the first submap of each trajectory, at its loaded
              pose.
  sigmas      PRIOR 0.1 x 6, connection 0.01 x 6, loop constraint 0.025 x 6 (multi_trajectory_optimizer.cc:66-81).
  huber       loop_huber (the reference's 1) on the loop constraints, connection_huber (default 0; the reference has 1) on the
              connections, none on a PRIOR.
  a connection is measured as target^-1 source of the LOADED poses, so its residual is zero at the start.
  hold_base   the base map's nodes are fixed and its PRIOR is left out.

A case (join_case) is two passes over one path, submaps `spacing` apart: the base map at the truth; the incremental map a little
beside it, loaded `drift` off (premultiplied: the whole map is displaced, as a second drive's own frame is).  Cross edges go from
base submap min(s, n_base - 1) to incremental submap s, for s from min(first_cross, n_inc - 1) on, measured as the truth with
N(0, rot_noise) rad / N(0, trans_noise) m noise."""
from __future__ import annotations

import functools

import numpy as np

import pose_graph_gps_ref as gps
import pose_graph_ref as ref
import pose_graph_robust_ref as robust

PRIOR_SIGMAS = np.full(6, 0.1)
CONNECTION_SIGMAS = np.full(6, 0.01)
LOOP_SIGMAS = np.full(6, 0.025)
DRIFT = ((0.0, 0.0, np.deg2rad(0.5)), (0.5, 0.5, 0.0))      # 0.5 m on x and on y (0.71 m), 0.5 degrees of yaw


def path_pose(k, spacing=4.0):
    """submap k of a pass: `spacing` along a gentle S-curve, small roll and pitch"""
    s = spacing * k
    yaw = 0.3 * np.sin(s / 40.0)
    return ref.make_pose((0.01 * np.sin(s / 9.0), 0.01 * np.cos(s / 7.0), yaw), (s, 6.0 * (1.0 - np.cos(s / 40.0)), 0.1 * np.sin(s / 15.0)))


BESIDE = ref.make_pose((0.0, 0.0, np.deg2rad(2.0)), (0.2, 0.3, 0.0))      # the second pass in the first one's submap frame


def join_case(n_base, n_inc, seed=1, first_cross=3, drift=DRIFT, rot_noise=0.002, trans_noise=0.01, spacing=4.0, wrong=None, every=1):
    """dict(base [n_base, 4, 4], inc_truth, inc_loaded [n_inc, 4, 4], cross [(base submap, incremental submap, Z)]).  wrong: an
    incremental submap whose cross edge is measured 3 m and 0.2 rad off instead.  every: a cross edge on every `every`-th submap only."""
    rng = np.random.default_rng(seed)
    base = np.stack([path_pose(k, spacing) for k in range(n_base)])
    inc_truth = np.stack([path_pose(k, spacing) @ BESIDE for k in range(n_inc)])
    D = ref.make_pose(*drift)
    inc_loaded = np.stack([D @ X for X in inc_truth])
    cross = []
    for s in range(min(first_cross, n_inc - 1), n_inc, every):
        b = min(s, n_base - 1)
        noise = np.eye(4)
        noise[:3, :3] = ref.exp_so3(rng.normal(size=3) * rot_noise)
        noise[:3, 3] = rng.normal(size=3) * trans_noise
        if wrong is not None and s == wrong:
            noise = ref.make_pose((0.0, 0.0, 0.2), (3.0, 0.0, 0.0))
        cross.append((b, s, ref.inv(base[b]) @ inc_truth[s] @ noise))
    return dict(base=base, inc_truth=inc_truth, inc_loaded=inc_loaded, cross=cross)


def assemble(case, hold_base=False, loop_huber=1.0, connection_huber=0.0):
    """the graph (pose_graph_gps_ref's dict plus huber) of a join; g["loops"]: the loop constraints' factor indices"""
    base, inc = case["base"], case["inc_loaded"]
    nb, ni = len(base), len(inc)
    poses = np.concatenate([base, inc])
    factors, huber, loops = [], [], []

    def connection(i, j):
        factors.append((gps.BETWEEN, i, j, gps.between_data(ref.inv(poses[i]) @ poses[j]), CONNECTION_SIGMAS))
        huber.append(connection_huber)
    for k in range(nb - 1):
        connection(k, k + 1)
    for b, s, Z in case["cross"]:                                          # (cross is in the order of its sources)
        loops.append(len(factors))
        factors.append((gps.BETWEEN, b, nb + s, gps.between_data(Z), LOOP_SIGMAS))
        huber.append(loop_huber)
    for k in range(ni - 1):
        connection(nb + k, nb + k + 1)
    if not hold_base:
        factors.append((gps.PRIOR, 0, 0, gps.prior_data(poses[0]), PRIOR_SIGMAS))
        huber.append(0.0)
    factors.append((gps.PRIOR, nb, nb, gps.prior_data(poses[nb]), PRIOR_SIGMAS))
    huber.append(0.0)
    fixed = np.zeros(nb + ni, np.uint8)
    if hold_base:
        fixed[:nb] = 1
    g = gps.make_graph(poses, fixed, factors)
    g.update(huber=np.array(huber), loops=loops, n_base=nb)
    return g


def optimize(g, solver="direct", max_iterations=50):
    """pose_graph_robust_ref.optimize, or pose_graph_gps_ref's when no factor has a threshold (the same loop; the entry PoseGraph::Optimize takes)"""
    return robust.optimize(g, max_iterations=max_iterations, solver=solver)


def mutual(case, poses, s):
    """base^-1 incremental at incremental submap s (against base submap min(s, n_base - 1)) under `poses` [n_base + n_inc, 4, 4]"""
    nb = len(case["base"])
    return ref.inv(poses[min(s, nb - 1)]) @ poses[nb + s]


def mutual_error(case, poses, s):
    """how far (m) the mutual pose at incremental submap s is from the truth's"""
    nb = len(case["base"])
    want = ref.inv(case["base"][min(s, nb - 1)]) @ case["inc_truth"][s]
    return float(np.linalg.norm(mutual(case, poses, s)[:3, 3] - want[:3, 3]))


def loaded(case):
    return np.concatenate([case["base"], case["inc_loaded"]])


# ---- the graphs the C++ and device tests solve as well -----------------------------------------------------------------------------
# 8 + 8, and the node counts at which the preconditioner's cyclic reduction changes level (65 and 66 nodes), with the joint between the
# trajectories at either end
PARITY = {"join8_8": (8, 8), "join63_2": (63, 2), "join64_1": (64, 1), "join1_64": (1, 64)}


@functools.lru_cache(maxsize=None)
def parity_case(name):
    return join_case(*PARITY[name])


@functools.lru_cache(maxsize=None)
def reference(name, hold_base):
    """(case, graph, the restatement's poses, its stats) -- computed once and left unchanged"""
    case = parity_case(name)
    g = assemble(case, hold_base=hold_base)
    poses, st = optimize(g)
    poses.setflags(write=False)
    return case, g, poses, st
