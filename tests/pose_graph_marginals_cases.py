"""Graphs shared by the marginal-covariance tests (CPU restatement, the kernel's routine under HostCtx, the device), all against
tests/pose_graph_marginals_ref.py.  Every graph is one of the existing case files'; the restatement's optimised poses are computed
once per process and left unchanged.

  stage cases         pose_graph_cases.stage_cases(): N = 2, 3, 5, 63, 64, 65, a missing chain edge, a fixed node in the middle,
                      reversed and doubled edges (the plain entry)
  circle64 / 240      the circle drives
  gps_chain23         PRIOR and POINT factors: a frame node held by its PRIOR alone (the *_factors entry)
  robust16            a ring with a wrong loop edge under an active Huber threshold (the *_robust entry)
  calib_ring16        HANDEYE factors and a calibration node (the *_calib entry)
  info_ring16         dense square-root informations on every BETWEEN, HANDEYE factors under Huber beside them (the *_info entry)
  two_nodes / prior   the two analytic cases: Sigma = diag(sigma^2)"""
import functools

import numpy as np

import pose_graph_calib_cases as calib_cases
import pose_graph_calib_ref as calib
import pose_graph_cases as base
import pose_graph_gps_cases as gps_cases
import pose_graph_gps_ref as gps
import pose_graph_info_cases as info_cases
import pose_graph_ref as ref
import pose_graph_robust_cases as robust_cases

PLAIN = sorted(base.stage_cases()) + ["circle64", "circle240"]
FACTOR = ["gps_chain23", "robust16", "calib_ring16", "info_ring16"]
ALL = PLAIN + FACTOR
ANALYTIC_SIGMAS = np.array([0.01, 0.02, 0.05, 0.1, 0.3, 0.7])


@functools.lru_cache(maxsize=None)
def optimised(name):
    """(graph, the restatement's optimised poses)"""
    if name in PLAIN:
        g, poses, _ = base.reference(name)
    elif name == "gps_chain23":
        g, poses, _ = gps_cases.reference("chain23_all")
    elif name == "robust16":
        g, poses, _, _ = robust_cases.reference("robust16")
    elif name == "calib_ring16":
        g, poses, _ = calib_cases.reference("ring16_free")
    elif name == "info_ring16":
        g, poses, _ = info_cases.reference("ring16_full")
    else:
        raise KeyError(name)
    return g, poses


@functools.lru_cache(maxsize=None)
def restated(name):
    """(H, fixed, cap, pcg_columns of every node, dense columns of every node) at the restatement's optimised poses: computed once"""
    import pose_graph_marginals_ref as mref
    g, poses = optimised(name)
    H, fixed, cap = mref.system(g, poses)
    q = list(range(len(poses)))
    return H, fixed, cap, mref.pcg_columns(H, fixed, q, cap), mref.dense_columns(mref.dense(H, fixed), q)


def two_nodes():
    """node 0 held, one BETWEEN measured exactly: at zero residual B = I / sigma, so Sigma_1 = diag(sigma^2)"""
    X0, X1 = ref.make_pose((0.1, -0.2, 0.7), (3.0, -1.0, 0.5)), ref.make_pose((-0.3, 0.1, 1.9), (7.0, 2.0, 0.2))
    return dict(poses=np.stack([X0, X1]), fixed=np.array([1, 0], np.uint8), edges=np.array([[0, 1]], np.int32), Z=np.stack([ref.inv(X0) @ X1]),
                sigmas=ANALYTIC_SIGMAS[None])


def prior_alone():
    """one free node held by a PRIOR around its own pose: Sigma_0 = the PRIOR's diag(sigma^2)"""
    X = ref.make_pose((0.2, 0.1, -1.1), (-4.0, 9.0, 1.0))
    return gps.make_graph([X], [0], [(gps.PRIOR, 0, 0, gps.prior_data(X), ANALYTIC_SIGMAS)])


def without_thresholds(g):
    out = dict(g)
    out["huber"] = np.zeros(len(g["kinds"]))
    return out
