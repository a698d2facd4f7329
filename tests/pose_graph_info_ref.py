"""The pose graph's BETWEEN factor with a full 6x6 square-root information (include/smhip.h, "Edge information")
restated in numpy, f64, on top of tests/pose_graph_calib_ref.py, which is imported as it is.  The device
(staticmapping_amd/csrc/pose_graph_kernel.h) is tested against this file.

  a graph     pose_graph_calib_ref's dict with one more entry: g["L"], per factor None or a [6, 6] L (the factor's information is
              L^T L).  A factor with an L must be a BETWEEN; its sigmas are not read.
  whitening   rw = L e,  A_w = L A,  B_w = L B,  s_f^2 = |L e|^2, with e, A, B the unwhitened residual and Jacobians of
              pose_graph_ref.  L = diag(1 / sigma) is the sigma form.
  Huber       pose_graph_robust_ref's term and weight on s_f, as for every factor.
  optimize    pose_graph_calib_ref.optimize's loop, line by line, with this cost and this linearisation."""
from __future__ import annotations

import numpy as np

import pose_graph_calib_ref as calib
import pose_graph_gps_ref as gps
import pose_graph_ref as ref
import pose_graph_robust_ref as robust

BETWEEN = calib.BETWEEN


def with_information(g, L):
    """a copy of the graph g with the square-root informations L: per factor None or [6, 6]"""
    out = dict(g)
    assert len(L) == len(g["kinds"])
    for k, l in enumerate(L):
        assert l is None or g["kinds"][k] == BETWEEN
    out["L"] = [None if l is None else np.asarray(l, np.float64).reshape(6, 6) for l in L]
    return out


def _L(g, k):
    return g["L"][k] if g.get("L") is not None else None


def linearize_plain(g, poses):
    F = len(g["kinds"])
    r, A, B = np.zeros((F, 6)), np.zeros((F, 6, 6)), np.zeros((F, 6, 6))
    for k in range(F):
        i, j = g["ij"][k]
        e, a, b = calib.factor_jacobians(g["kinds"][k], poses[i], poses[j], g["data"][k])
        L = _L(g, k)
        if L is not None:
            r[k], A[k], B[k] = L @ e, L @ a, L @ b
        else:
            w = gps._whiten(g["kinds"][k], g["sigmas"][k])
            r[k], A[k], B[k] = e * w, a * w[:, None], b * w[:, None]
    return r, A, B


def norm2(g, poses, k):
    L = _L(g, k)
    if L is None:
        return calib.norm2(g, poses, k)
    i, j = g["ij"][k]
    e = calib.factor_residual(g["kinds"][k], poses[i], poses[j], g["data"][k])
    return float(np.sum((L @ e) ** 2))


def cost(g, poses):
    hub = robust.thresholds(g)
    return sum(float(robust.term(hub[k], norm2(g, poses, k))) for k in range(len(g["kinds"])))


def report(g, poses):
    hub = robust.thresholds(g)
    s2 = np.array([norm2(g, poses, k) for k in range(len(hub))])
    return (np.sqrt(s2), np.array([robust.weight(k, v) for k, v in zip(hub, s2)]).reshape(-1), np.array([robust.term(k, v) for k, v in zip(hub, s2)]).reshape(-1))


def linearize(g, poses):
    r, A, B = linearize_plain(g, poses)
    hub = robust.thresholds(g)
    w = np.ones(len(hub))
    for k in range(len(hub)):
        w[k] = robust.weight(hub[k], float(np.sum(r[k] ** 2)))
        if w[k] < 1.0:
            q = np.sqrt(w[k])
            r[k], A[k], B[k] = r[k] * q, A[k] * q, B[k] * q
    return r, A, B, w


def assemble(g, poses):
    edges = [(int(i), int(j)) for i, j in g["ij"]]
    r, A, B, _ = linearize(g, poses)
    return ref.assemble(len(poses), g["fixed"], edges, r, A, B)


def optimize(g, max_iterations=50, solver="direct"):
    """pose_graph_calib_ref.optimize's loop with this module's cost and linearisation: (poses, stats); solver "direct" or "pcg\""""
    poses = np.array(g["poses"], np.float64)
    n, fixed = len(poses), g["fixed"]
    cap = 12 * calib.non_chain_edges(g) + 64
    c0 = cost(g, poses)
    st = dict(initial_cost=c0, accepted=0, rejected=0, pcg_iterations=0, pcg_max=0, stop=ref.STOP_MAX_ITERATIONS)
    lam, lin = 0.0, None
    for _ in range(max_iterations):
        if lin is None:
            lin = assemble(g, poses)
        H, grad = lin
        Hl = ref.damped(H, lam, fixed)
        if solver == "direct":
            d = np.linalg.solve(Hl, -grad)
        else:
            d, its = ref.pcg(Hl, ref.chain_part(Hl), grad, cap)
            st["pcg_iterations"] += its
            st["pcg_max"] = max(st["pcg_max"], its)
        cand = np.stack([poses[k] if fixed[k] else ref.retract(poses[k], d[6 * k:6 * k + 6]) for k in range(n)])
        c1 = cost(g, cand)
        if np.max(np.abs(d)) < ref.STEP_TOL:
            poses, c0 = cand, c1
            st["accepted"] += 1
            st["stop"] = ref.STOP_STEP
            break
        band = ref.COST_TOL * c0 + ref.COST_NOISE * np.sqrt(c0)
        if c1 <= c0 + band:
            dec = c0 - c1
            poses, c0, lin = cand, c1, None
            st["accepted"] += 1
            lam = 0.0 if lam <= ref.LAMBDA_FIRST else lam / 10.0
            if dec <= band:
                st["stop"] = ref.STOP_COST
                break
        else:
            st["rejected"] += 1
            lam = ref.LAMBDA_FIRST if lam == 0.0 else 10.0 * lam
            if lam > ref.LAMBDA_MAX:
                st["stop"] = ref.STOP_DAMPING
                break
    st["final_cost"] = c0
    st["damping"] = lam
    return poses, st
