"""ctypes view of the device pose-graph optimiser (include/smhip.h, `smhip_pose_graph_*`): what back_end::IsamOptimizer asks of GTSAM
in the reference (back_end/isam_optimizer.{h,cc}) -- rigid poses, between-factors, fixed nodes, and the PRIOR and POINT factors behind its GPS / ENU factors
(*_factors below), any of them with a Huber threshold (*_robust), and the HANDEYE factor behind its odometry calibration (*_calib) -- as one kernel launch per optimisation.  The definition is DESIGN.md section 6 ("Pose graph").  No compute happens in Python."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi

MAX_NODES, MAX_EDGES = 8192, 32768
BETWEEN, PRIOR, POINT, HANDEYE = 0, 1, 2, 3
STOP_REASONS = {1: "step", 2: "cost", 3: "max_iterations", 4: "damping", 5: "numeric"}
c_uint8_p = ctypes.POINTER(ctypes.c_uint8)


class PoseGraphRefused(ValueError):
    """smhip_pose_graph_plan refused the graph; .status is the smhip_status"""

    def __init__(self, status, text):
        super().__init__(text)
        self.status = status


def _arrays(poses, fixed, edges, Z, sigmas):
    poses = np.asarray(poses, np.float64)
    n = len(poses)
    edges = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
    Z = np.asarray(Z, np.float64).reshape(-1, 4, 4)
    if poses.shape[1:] != (4, 4) or len(Z) != len(edges):
        raise ValueError("poses [N, 4, 4], edges [E, 2], Z [E, 4, 4]")
    if fixed is None:
        fixed = np.zeros(n, np.uint8)
        fixed[:1] = 1
    fixed = np.ascontiguousarray(np.asarray(fixed).astype(bool).astype(np.uint8))
    if len(fixed) != n:
        raise ValueError("one fixed flag per pose")
    if sigmas is not None:
        sigmas = np.ascontiguousarray(np.broadcast_to(np.asarray(sigmas, np.float64), (len(edges), 6)))
    # the ABI's 4x4 are column-major: the transpose of numpy's rows
    return (np.ascontiguousarray(poses.transpose(0, 2, 1)), fixed, edges, np.ascontiguousarray(Z.transpose(0, 2, 1)), sigmas)


def _ptr(a, kind):
    return None if a is None or a.size == 0 else a.ctypes.data_as(kind)


def plan(poses, edges, Z, fixed=None, sigmas=None):
    """The host half of optimize(), which needs no device: (csr_offsets [N + 1], csr_edges [2 E]) -- node k's edges, ascending, at
    csr_edges[csr_offsets[k]:csr_offsets[k + 1]] -- or PoseGraphRefused with the reason."""
    P, F, E, Zc, S = _arrays(poses, fixed, edges, Z, sigmas)
    off = np.zeros(len(P) + 1, np.int32)
    inc = np.zeros(max(2 * len(E), 1), np.int32)
    why = ctypes.create_string_buffer(256)
    s = _capi.load_library().smhip_pose_graph_plan(len(P), _ptr(P, _capi.c_double_p), _ptr(F, c_uint8_p), len(E), _ptr(E, _capi.c_int32_p),
                                                   _ptr(Zc, _capi.c_double_p), _ptr(S, _capi.c_double_p), off.ctypes.data_as(_capi.c_int32_p),
                                                   inc.ctypes.data_as(_capi.c_int32_p), why, len(why))
    if s != 0:
        raise PoseGraphRefused(s, why.value.decode())
    return off, inc[:2 * len(E)]


def optimize(matcher, poses, edges, Z, fixed=None, sigmas=None, max_iterations: int | None = None):
    """Minimise sum |e / sigma|^2 over the free poses from `poses` ([N, 4, 4]); edges [E, 2] of (i, j) with Z [E, 4, 4] the measured
    X_i^-1 X_j; fixed: N flags (default: node 0 alone); sigmas: [6] or [E, 6], rotation first (default 0.1 x 3, 0.15 x 3).
    Returns (poses [N, 4, 4], stats dict).  `matcher`: any handle owner of this package (e.g. IcpFastHip)."""
    P, F, E, Zc, S = _arrays(poses, fixed, edges, Z, sigmas)
    lib = matcher._lib
    o = _capi.PoseGraphOptions()
    lib.smhip_pose_graph_default_options(ctypes.byref(o))
    if max_iterations is not None:
        o.max_iterations = max_iterations
    st = _capi.PoseGraphStats()
    matcher._check(lib.smhip_pose_graph_optimize(matcher._h, len(P), _ptr(P, _capi.c_double_p), _ptr(F, c_uint8_p), len(E), _ptr(E, _capi.c_int32_p),
                                                 _ptr(Zc, _capi.c_double_p), _ptr(S, _capi.c_double_p), ctypes.byref(o), ctypes.byref(st)))
    stats = {name: getattr(st, name) for name, _ in _capi.PoseGraphStats._fields_}
    stats["stop"] = STOP_REASONS.get(st.stop_reason, "?")
    return np.ascontiguousarray(P.transpose(0, 2, 1)), stats


def factor_data(kind, *parts):
    """The 16 doubles of one factor: (BETWEEN, Z [4, 4]), (PRIOR, P [4, 4]), (HANDEYE, Z [4, 4]) -- column-major -- or (POINT, lever [3], point [3])"""
    out = np.zeros(16)
    if kind == POINT:
        out[:3], out[3:6] = parts
    else:
        out[:] = np.asarray(parts[0], np.float64).T.ravel()
    return out


def _factor_arrays(poses, fixed, kinds, ij, data, sigmas):
    poses = np.asarray(poses, np.float64)
    n = len(poses)
    ij = np.ascontiguousarray(np.asarray(ij, np.int32).reshape(-1, 2))
    data = np.ascontiguousarray(np.asarray(data, np.float64).reshape(-1, 16))
    if kinds is not None:
        kinds = np.ascontiguousarray(np.asarray(kinds, np.uint8).reshape(-1))
    if poses.shape[1:] != (4, 4) or len(data) != len(ij) or (kinds is not None and len(kinds) != len(ij)):
        raise ValueError("poses [N, 4, 4], kinds [F], ij [F, 2], data [F, 16]")
    if fixed is None:
        fixed = np.zeros(n, np.uint8)
    fixed = np.ascontiguousarray(np.asarray(fixed).astype(bool).astype(np.uint8))
    if len(fixed) != n:
        raise ValueError("one fixed flag per pose")
    if sigmas is not None:
        sigmas = np.ascontiguousarray(np.broadcast_to(np.asarray(sigmas, np.float64), (len(ij), 6)))
    return np.ascontiguousarray(poses.transpose(0, 2, 1)), fixed, kinds, ij, data, sigmas


def plan_factors(poses, kinds, ij, data, fixed=None, sigmas=None):
    """plan() for factors of any kind (include/smhip.h, "Factor kinds"): kinds [F] of BETWEEN / PRIOR / POINT or None for all BETWEEN,
    ij [F, 2], data [F, 16] as factor_data() lays it out, fixed: N flags (default: none), sigmas [F, 6].  Returns (csr_offsets [N + 1],
    csr_edges [csr_offsets[N]]: a PRIOR is listed once) or raises PoseGraphRefused."""
    P, F, K, E, D, S = _factor_arrays(poses, fixed, kinds, ij, data, sigmas)
    off = np.zeros(len(P) + 1, np.int32)
    inc = np.zeros(max(2 * len(E), 1), np.int32)
    why = ctypes.create_string_buffer(256)
    s = _capi.load_library().smhip_pose_graph_plan_factors(len(P), _ptr(P, _capi.c_double_p), _ptr(F, c_uint8_p), len(E), _ptr(K, c_uint8_p),
                                                           _ptr(E, _capi.c_int32_p), _ptr(D, _capi.c_double_p), _ptr(S, _capi.c_double_p),
                                                           off.ctypes.data_as(_capi.c_int32_p), inc.ctypes.data_as(_capi.c_int32_p), why, len(why))
    if s != 0:
        raise PoseGraphRefused(s, why.value.decode())
    return off, inc[:off[-1]]


def optimize_factors(matcher, poses, kinds, ij, data, fixed=None, sigmas=None, max_iterations: int | None = None):
    """optimize() for factors of any kind; the arguments of plan_factors().  Returns (poses [N, 4, 4], stats dict); last() serves
    this call too, with n_edges = the factor count."""
    P, F, K, E, D, S = _factor_arrays(poses, fixed, kinds, ij, data, sigmas)
    lib = matcher._lib
    o = _capi.PoseGraphOptions()
    lib.smhip_pose_graph_default_options(ctypes.byref(o))
    if max_iterations is not None:
        o.max_iterations = max_iterations
    st = _capi.PoseGraphStats()
    matcher._check(lib.smhip_pose_graph_optimize_factors(matcher._h, len(P), _ptr(P, _capi.c_double_p), _ptr(F, c_uint8_p), len(E), _ptr(K, c_uint8_p),
                                                         _ptr(E, _capi.c_int32_p), _ptr(D, _capi.c_double_p), _ptr(S, _capi.c_double_p),
                                                         ctypes.byref(o), ctypes.byref(st)))
    stats = {name: getattr(st, name) for name, _ in _capi.PoseGraphStats._fields_}
    stats["stop"] = STOP_REASONS.get(st.stop_reason, "?")
    return np.ascontiguousarray(P.transpose(0, 2, 1)), stats


def _huber(huber, n_factors):
    if huber is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(huber, np.float64), (n_factors,)))


def plan_robust(poses, kinds, ij, data, fixed=None, sigmas=None, huber=None):
    """plan_factors() plus huber: one Huber threshold per factor ([F] or a scalar; 0 = none) or None for none at all (include/smhip.h,
    "Robust factors").  A threshold that is negative or not finite raises PoseGraphRefused."""
    P, F, K, E, D, S = _factor_arrays(poses, fixed, kinds, ij, data, sigmas)
    H = _huber(huber, len(E))
    off = np.zeros(len(P) + 1, np.int32)
    inc = np.zeros(max(2 * len(E), 1), np.int32)
    why = ctypes.create_string_buffer(256)
    s = _capi.load_library().smhip_pose_graph_plan_robust(len(P), _ptr(P, _capi.c_double_p), _ptr(F, c_uint8_p), len(E), _ptr(K, c_uint8_p),
                                                          _ptr(E, _capi.c_int32_p), _ptr(D, _capi.c_double_p), _ptr(S, _capi.c_double_p),
                                                          _ptr(H, _capi.c_double_p), off.ctypes.data_as(_capi.c_int32_p),
                                                          inc.ctypes.data_as(_capi.c_int32_p), why, len(why))
    if s != 0:
        raise PoseGraphRefused(s, why.value.decode())
    return off, inc[:off[-1]]


def optimize_robust(matcher, poses, kinds, ij, data, fixed=None, sigmas=None, huber=None, max_iterations: int | None = None):
    """optimize_factors() with Huber thresholds; the arguments of plan_robust().  Returns (poses [N, 4, 4], stats dict); last() then
    gives the weighted rows and last_robust() every factor's norm, weight and cost term."""
    P, F, K, E, D, S = _factor_arrays(poses, fixed, kinds, ij, data, sigmas)
    H = _huber(huber, len(E))
    lib = matcher._lib
    o = _capi.PoseGraphOptions()
    lib.smhip_pose_graph_default_options(ctypes.byref(o))
    if max_iterations is not None:
        o.max_iterations = max_iterations
    st = _capi.PoseGraphStats()
    matcher._check(lib.smhip_pose_graph_optimize_robust(matcher._h, len(P), _ptr(P, _capi.c_double_p), _ptr(F, c_uint8_p), len(E), _ptr(K, c_uint8_p),
                                                        _ptr(E, _capi.c_int32_p), _ptr(D, _capi.c_double_p), _ptr(S, _capi.c_double_p),
                                                        _ptr(H, _capi.c_double_p), ctypes.byref(o), ctypes.byref(st)))
    stats = {name: getattr(st, name) for name, _ in _capi.PoseGraphStats._fields_}
    stats["stop"] = STOP_REASONS.get(st.stop_reason, "?")
    return np.ascontiguousarray(P.transpose(0, 2, 1)), stats


def plan_calib(poses, kinds, ij, data, fixed=None, sigmas=None, huber=None):
    """plan_robust() that also accepts HANDEYE factors (include/smhip.h, "Odometry calibration factor"): ij = (frame node, calibration
    node), data = factor_data(HANDEYE, Z) with Z the odometer's pose.  A free calibration node without a PRIOR raises PoseGraphRefused."""
    P, F, K, E, D, S = _factor_arrays(poses, fixed, kinds, ij, data, sigmas)
    H = _huber(huber, len(E))
    off = np.zeros(len(P) + 1, np.int32)
    inc = np.zeros(max(2 * len(E), 1), np.int32)
    why = ctypes.create_string_buffer(256)
    s = _capi.load_library().smhip_pose_graph_plan_calib(len(P), _ptr(P, _capi.c_double_p), _ptr(F, c_uint8_p), len(E), _ptr(K, c_uint8_p),
                                                         _ptr(E, _capi.c_int32_p), _ptr(D, _capi.c_double_p), _ptr(S, _capi.c_double_p),
                                                         _ptr(H, _capi.c_double_p), off.ctypes.data_as(_capi.c_int32_p),
                                                         inc.ctypes.data_as(_capi.c_int32_p), why, len(why))
    if s != 0:
        raise PoseGraphRefused(s, why.value.decode())
    return off, inc[:off[-1]]


def optimize_calib(matcher, poses, kinds, ij, data, fixed=None, sigmas=None, huber=None, max_iterations: int | None = None):
    """optimize_robust() that also accepts HANDEYE factors; the arguments of plan_calib().  Returns (poses [N, 4, 4], stats dict); last()
    and last_robust() serve this call too."""
    P, F, K, E, D, S = _factor_arrays(poses, fixed, kinds, ij, data, sigmas)
    H = _huber(huber, len(E))
    lib = matcher._lib
    o = _capi.PoseGraphOptions()
    lib.smhip_pose_graph_default_options(ctypes.byref(o))
    if max_iterations is not None:
        o.max_iterations = max_iterations
    st = _capi.PoseGraphStats()
    matcher._check(lib.smhip_pose_graph_optimize_calib(matcher._h, len(P), _ptr(P, _capi.c_double_p), _ptr(F, c_uint8_p), len(E), _ptr(K, c_uint8_p),
                                                       _ptr(E, _capi.c_int32_p), _ptr(D, _capi.c_double_p), _ptr(S, _capi.c_double_p),
                                                       _ptr(H, _capi.c_double_p), ctypes.byref(o), ctypes.byref(st)))
    stats = {name: getattr(st, name) for name, _ in _capi.PoseGraphStats._fields_}
    stats["stop"] = STOP_REASONS.get(st.stop_reason, "?")
    return np.ascontiguousarray(P.transpose(0, 2, 1)), stats


def _info(sqrt_information, n_factors):
    """sqrt_information: None, or one entry per factor -- None / a [6, 6] L (row-major; the factor's information is L^T L) -- as
    (info_index [F] int32, sqrt_info [K, 36]) of the ABI"""
    if sqrt_information is None:
        return None, None
    if len(sqrt_information) != n_factors:
        raise ValueError("one square-root information (or None) per factor")
    index = np.full(n_factors, -1, np.int32)
    rows = []
    for e, L in enumerate(sqrt_information):
        if L is not None:
            index[e] = len(rows)
            rows.append(np.asarray(L, np.float64).reshape(36))
    return index, (np.ascontiguousarray(np.stack(rows)) if rows else None)


def plan_info(poses, kinds, ij, data, fixed=None, sigmas=None, huber=None, sqrt_information=None, info_index=None, sqrt_info=None):
    """plan_calib() plus sqrt_information: per factor None or the 6x6 L a BETWEEN is whitened by in place of its sigmas (include/smhip.h,
    "Edge information").  info_index / sqrt_info give the ABI's two arrays directly instead.  An index out of range, an L on a factor
    that is no BETWEEN, a non-finite or singular L raise PoseGraphRefused."""
    P, F, K, E, D, S = _factor_arrays(poses, fixed, kinds, ij, data, sigmas)
    H = _huber(huber, len(E))
    if sqrt_information is not None:
        info_index, sqrt_info = _info(sqrt_information, len(E))
    I = None if info_index is None else np.ascontiguousarray(np.asarray(info_index, np.int32).reshape(-1))
    Ls = None if sqrt_info is None else np.ascontiguousarray(np.asarray(sqrt_info, np.float64).reshape(-1, 36))
    off = np.zeros(len(P) + 1, np.int32)
    inc = np.zeros(max(2 * len(E), 1), np.int32)
    why = ctypes.create_string_buffer(256)
    s = _capi.load_library().smhip_pose_graph_plan_info(len(P), _ptr(P, _capi.c_double_p), _ptr(F, c_uint8_p), len(E), _ptr(K, c_uint8_p),
                                                        _ptr(E, _capi.c_int32_p), _ptr(D, _capi.c_double_p), _ptr(S, _capi.c_double_p),
                                                        _ptr(H, _capi.c_double_p), _ptr(I, _capi.c_int32_p), _ptr(Ls, _capi.c_double_p),
                                                        off.ctypes.data_as(_capi.c_int32_p), inc.ctypes.data_as(_capi.c_int32_p), why, len(why))
    if s != 0:
        raise PoseGraphRefused(s, why.value.decode())
    return off, inc[:off[-1]]


def optimize_info(matcher, poses, kinds, ij, data, fixed=None, sigmas=None, huber=None, sqrt_information=None, info_index=None, sqrt_info=None,
                  max_iterations: int | None = None):
    """optimize_calib() in which a BETWEEN may carry a full 6x6 square-root information; the arguments of plan_info().  Without one
    every output has the bits of optimize_calib().  Returns (poses [N, 4, 4], stats dict); last() and last_robust() serve this call too."""
    P, F, K, E, D, S = _factor_arrays(poses, fixed, kinds, ij, data, sigmas)
    H = _huber(huber, len(E))
    if sqrt_information is not None:
        info_index, sqrt_info = _info(sqrt_information, len(E))
    I = None if info_index is None else np.ascontiguousarray(np.asarray(info_index, np.int32).reshape(-1))
    Ls = None if sqrt_info is None else np.ascontiguousarray(np.asarray(sqrt_info, np.float64).reshape(-1, 36))
    lib = matcher._lib
    o = _capi.PoseGraphOptions()
    lib.smhip_pose_graph_default_options(ctypes.byref(o))
    if max_iterations is not None:
        o.max_iterations = max_iterations
    st = _capi.PoseGraphStats()
    matcher._check(lib.smhip_pose_graph_optimize_info(matcher._h, len(P), _ptr(P, _capi.c_double_p), _ptr(F, c_uint8_p), len(E), _ptr(K, c_uint8_p),
                                                      _ptr(E, _capi.c_int32_p), _ptr(D, _capi.c_double_p), _ptr(S, _capi.c_double_p),
                                                      _ptr(H, _capi.c_double_p), _ptr(I, _capi.c_int32_p), _ptr(Ls, _capi.c_double_p),
                                                      ctypes.byref(o), ctypes.byref(st)))
    stats = {name: getattr(st, name) for name, _ in _capi.PoseGraphStats._fields_}
    stats["stop"] = STOP_REASONS.get(st.stop_reason, "?")
    return np.ascontiguousarray(P.transpose(0, 2, 1)), stats


def last_robust(matcher, n_factors: int):
    """The report of the last optimise call on the handle, whichever it was, which had n_factors factors (another count is refused): dict(norm [F]
    = s_f, weight [F] = w_f, cost [F] = the cost term) at the poses that call ended at.  After a call without thresholds every weight is 1."""
    norm, weight, cost = np.zeros(n_factors), np.zeros(n_factors), np.zeros(n_factors)
    matcher._check(matcher._lib.smhip_pose_graph_last_robust(matcher._h, n_factors, _ptr(norm, _capi.c_double_p), _ptr(weight, _capi.c_double_p),
                                                             _ptr(cost, _capi.c_double_p)))
    return dict(norm=norm, weight=weight, cost=cost)


def last(matcher, n_nodes: int, n_edges: int, v=None):
    """Parity hook: the first linearisation of the last optimize() on the handle, which had n_nodes and n_edges (other sizes are refused).  Returns dict(r [E, 6]
    whitened residuals, A, B [E, 6, 6] whitened, g [N, 6], minv_v [N, 6] = M^-1 v or None without v).  After optimize_robust() the rows are the weighted ones."""
    r = np.zeros((n_edges, 6))
    A = np.zeros((n_edges, 6, 6))
    B = np.zeros((n_edges, 6, 6))
    g = np.zeros((n_nodes, 6))
    out = None
    if v is not None:
        v = np.ascontiguousarray(np.asarray(v, np.float64).reshape(n_nodes, 6))
        out = np.zeros((n_nodes, 6))
    matcher._check(matcher._lib.smhip_pose_graph_last(matcher._h, n_nodes, n_edges, _ptr(r, _capi.c_double_p), _ptr(A, _capi.c_double_p), _ptr(B, _capi.c_double_p),
                                                      _ptr(g, _capi.c_double_p), _ptr(v, _capi.c_double_p), _ptr(out, _capi.c_double_p)))
    return dict(r=r, A=A, B=B, g=g, minv_v=out)


def marginals(matcher, n_nodes: int, query, rows=None, max_workgroups: int | None = None):
    """Marginal covariances of the last optimise call on the handle, whichever it was (include/smhip.h, "Marginal covariances"): for every
    node in `query`, Sigma_k = the symmetrised diagonal block of H^-1 at the poses that call ended at, in the optimiser's tangent chart
    (rotation first; the translation part in the node's body frame), relative to the held nodes or PRIORs; zeros for a fixed node.
    rows: node indices whose cross blocks [H^-1]_{r, k} are wanted too.  Returns (cov [Q, 6, 6], blocks [Q, R, 6, 6] or None, stats dict)."""
    q = np.ascontiguousarray(np.asarray(query, np.int32).reshape(-1))
    r = None if rows is None else np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1))
    cov = np.zeros((len(q), 6, 6))
    blocks = None if r is None else np.zeros((len(q), len(r), 6, 6))
    lib = matcher._lib
    o = _capi.PoseGraphMarginalsOptions()
    lib.smhip_pose_graph_marginals_default_options(ctypes.byref(o))
    if max_workgroups is not None:
        o.max_workgroups = max_workgroups
    st = _capi.PoseGraphMarginalsStats()
    matcher._check(lib.smhip_pose_graph_marginals(matcher._h, n_nodes, len(q), _ptr(q, _capi.c_int32_p), _ptr(cov, _capi.c_double_p),
                                                  0 if r is None else len(r), _ptr(r, _capi.c_int32_p), _ptr(blocks, _capi.c_double_p),
                                                  ctypes.byref(o), ctypes.byref(st)))
    return cov, blocks, {name: getattr(st, name) for name, _ in _capi.PoseGraphMarginalsStats._fields_}
