"""Huber-robust factors of the pose graph ("Pose graph", Robust factors), restated in numpy, f64, on top of
tests/pose_graph_ref.py and tests/pose_graph_gps_ref.py, which are imported as they are.  The device
(staticmapping_amd/csrc/pose_graph_kernel.h) is tested against this file.

  a graph     pose_graph_gps_ref's dict plus huber [F]: one threshold k_f >= 0 per factor, 0 = none.
  s_f^2       the sum of (e / sigma)^2 over the rows the factor reads: six, or three for a POINT.
  cost term   s_f^2 when k_f == 0 or s_f^2 <= k_f^2, else 2 k_f s_f - k_f^2: twice the Huber loss, so that a graph without
              thresholds has pose_graph_gps_ref's cost.
  weight      w_f = 1 in the first case, k_f / s_f in the second.
  linearise   pose_graph_gps_ref's whitened r, A and B, then times sqrt(w_f) -- only where w_f < 1.  J^T r is then the exact
              gradient of half the cost and H = sum w J^T J (GTSAM's Robust::WhitenSystem).
  optimize    pose_graph_gps_ref.optimize's loop, line by line, with this cost and this linearisation; nothing else differs.
  report      per factor s_f, w_f and the cost term at given poses."""
from __future__ import annotations

import numpy as np

import pose_graph_gps_ref as gps
import pose_graph_ref as ref


def thresholds(g):
    h = g.get("huber")
    return np.zeros(len(g["kinds"])) if h is None else np.asarray(h, np.float64)


def norm2(g, poses, k):
    """s_f^2 of factor k, summed as pose_graph_gps_ref.cost sums it"""
    i, j = g["ij"][k]
    e = gps.factor_residual(g["kinds"][k], poses[i], poses[j], g["data"][k])
    return float(np.sum((e * gps._whiten(g["kinds"][k], g["sigmas"][k])) ** 2))


def term(k, s2):
    """the cost term of a factor with threshold k and squared norm s2"""
    if k == 0.0 or s2 <= k * k:
        return s2
    return 2.0 * k * np.sqrt(s2) - k * k


def weight(k, s2):
    if k == 0.0 or s2 <= k * k:
        return 1.0
    return k / np.sqrt(s2)


def cost(g, poses):
    hub = thresholds(g)
    s = 0.0
    for k in range(len(g["kinds"])):
        s += float(term(hub[k], norm2(g, poses, k)))
    return s


def report(g, poses):
    """(norm [F], weight [F], cost term [F]) at `poses`"""
    hub = thresholds(g)
    s2 = np.array([norm2(g, poses, k) for k in range(len(hub))])
    return (np.sqrt(s2), np.array([weight(k, v) for k, v in zip(hub, s2)]).reshape(-1), np.array([term(k, v) for k, v in zip(hub, s2)]).reshape(-1))


def linearize(g, poses):
    """whitened and weighted r [F, 6], A [F, 6, 6], B [F, 6, 6] at `poses`, and the weights [F]"""
    r, A, B = gps.linearize(g, poses)
    hub = thresholds(g)
    w = np.ones(len(hub))
    for k in range(len(hub)):
        w[k] = weight(hub[k], float(np.sum(r[k] ** 2)))
        if w[k] < 1.0:
            q = np.sqrt(w[k])
            r[k], A[k], B[k] = r[k] * q, A[k] * q, B[k] * q
    return r, A, B, w


def assemble(g, poses, sparse=False):
    n = len(poses)
    edges = [(int(i), int(j)) for i, j in g["ij"]]
    r, A, B, _ = linearize(g, poses)
    return (ref.assemble_sparse if sparse else ref.assemble)(n, g["fixed"], edges, r, A, B)


def gradient_norm(g, poses):
    return float(np.linalg.norm(assemble(g, poses)[1]))


def optimize(g, max_iterations=50, solver="direct"):
    """pose_graph_gps_ref.optimize's loop, line by line, with the robust cost and linearisation: (poses, stats).  solver: "direct",
    "pcg", "sparse" (and "sparse_pcg").  stats also keeps, per accepted step that went through the cost rule, decrease / band."""
    poses = np.array(g["poses"], np.float64)
    n, fixed = len(poses), g["fixed"]
    cap = 12 * gps.non_chain_edges(g) + 64
    c0 = cost(g, poses)
    st = dict(initial_cost=c0, accepted=0, rejected=0, pcg_iterations=0, pcg_max=0, pcg_each=[], stop=ref.STOP_MAX_ITERATIONS, costs=[c0], decrease_over_band=[])
    lam, lin = 0.0, None
    for _ in range(max_iterations):
        if lin is None:
            lin = assemble(g, poses, sparse=solver.startswith("sparse"))
        H, grad = lin
        Hl = ref.damped_sparse(H, lam, fixed) if solver.startswith("sparse") else ref.damped(H, lam, fixed)
        if solver == "direct":
            d = np.linalg.solve(Hl, -grad)
        elif solver == "sparse":
            import scipy.sparse.linalg as spl
            d = spl.spsolve(Hl, -grad)
        else:
            d, its = gps.pcg_sparse(Hl, gps.chain_part_sparse(Hl), grad, cap) if solver == "sparse_pcg" else ref.pcg(Hl, ref.chain_part(Hl), grad, cap)
            st["pcg_iterations"] += its
            st["pcg_max"] = max(st["pcg_max"], its)
            st["pcg_each"].append(its)
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
            st["decrease_over_band"].append(dec / band if band > 0.0 else np.inf)
            poses, c0, lin = cand, c1, None
            st["accepted"] += 1
            st["costs"].append(c1)
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
