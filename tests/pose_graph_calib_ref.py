"""The pose graph's HANDEYE factor -- the reference's odometry calibration factor through ODOM_CALIB_KEY (back_end/isam_optimizer.cc:84-93,
153-162, 209-224, 361-367) -- restated in numpy, f64 ("Pose graph", Odometry calibration factor), on top of
tests/pose_graph_ref.py, tests/pose_graph_gps_ref.py and tests/pose_graph_robust_ref.py, which are imported as they are.  The device
(staticmapping_amd/csrc/pose_graph_kernel.h) is tested against this file.

  HANDEYE     between a frame node i (pose X) and a calibration node j != i (pose T): data = Z, a rigid pose, column-major 4x4, the
              odometer's pose relative to its first reading.  h = T^-1 X T,  E = Z^-1 h,  e = [Log_SO3(R_E); t_E] (rotation first),
              whitened by six sigmas.  The model assumes that the frame node of the first reading is at the identity.
  Jacobians   under the retraction R <- R Exp(dw), t <- t + R dv:  X Exp(xi) turns h into h Exp(Ad(T^-1) xi) and T Exp(zeta) turns it
              into h Exp((I - Ad(h^-1)) zeta), with Ad(G) = [R_G, 0; hat(t_G) R_G, R_G]; a right perturbation of h moves e by
              B_h = [Jr^-1(e_w), 0; 0, R_E].  So  A = de/dxi_i = B_h Ad(T^-1),  B = de/dxi_j = B_h (I - Ad(h^-1)).
              B vanishes where h is the identity and is rank-deficient for planar motion.
  a graph     pose_graph_robust_ref's dict (huber optional); the calibration node comes after the chain and before a GPS frame node.
  non-chain   BETWEEN, POINT and HANDEYE factors with |i - j| != 1.
  Huber       pose_graph_robust_ref's term and weight, s_f^2 over the six rows.
  optimize    pose_graph_robust_ref.optimize's loop, line by line, with this cost and this linearisation."""
from __future__ import annotations

import numpy as np

import pose_graph_gps_ref as gps
import pose_graph_ref as ref
import pose_graph_robust_ref as robust

BETWEEN, PRIOR, POINT, HANDEYE = 0, 1, 2, 3
ODOM_SIGMAS = np.array([0.2, 0.2, 0.2, 1.5, 1.5, 2.0])                 # odom_noise_model_, :92-93
ODOM_HUBER = 1.0                                                       # :90-91
CALIB_PRIOR_SIGMAS = np.array([0.5, 0.5, 1.5, 0.1, 0.1, 0.1])          # odom_tf_noise_model_ with enable_extrinsic_calib, :85-86


def handeye_data(Z):
    return np.asarray(Z, np.float64).T.ravel().copy()


def adjoint(G):
    """Ad(G) for xi = [dw; dv]: G Exp(xi) G^-1 = Exp(Ad(G) xi)"""
    R, t = G[:3, :3], G[:3, 3]
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = R
    Ad[3:, :3] = ref.hat(t) @ R
    Ad[3:, 3:] = R
    return Ad


def handeye_residual(X, T, Z):
    E = ref.inv(Z) @ (ref.inv(T) @ X @ T)
    return np.concatenate([ref.log_so3(E[:3, :3]), E[:3, 3]])


def handeye_jacobians(X, T, Z):
    """e, A = de/dxi_X, B = de/dxi_T, unwhitened"""
    h = ref.inv(T) @ X @ T
    E = ref.inv(Z) @ h
    e = np.concatenate([ref.log_so3(E[:3, :3]), E[:3, 3]])
    Bh = np.zeros((6, 6))
    Bh[:3, :3] = ref.jr_inv(e[:3])
    Bh[3:, 3:] = E[:3, :3]
    return e, Bh @ adjoint(ref.inv(T)), Bh @ (np.eye(6) - adjoint(ref.inv(h)))


def factor_jacobians(kind, Xi, Xj, data):
    if kind == HANDEYE:
        return handeye_jacobians(Xi, Xj, gps._mat(data))
    return gps.factor_jacobians(kind, Xi, Xj, data)


def factor_residual(kind, Xi, Xj, data):
    if kind == HANDEYE:
        return handeye_residual(Xi, Xj, gps._mat(data))
    return gps.factor_residual(kind, Xi, Xj, data)


def linearize_plain(g, poses):
    """pose_graph_gps_ref.linearize over the four kinds: whitened r [F, 6], A [F, 6, 6], B [F, 6, 6] at `poses`"""
    F = len(g["kinds"])
    r, A, B = np.zeros((F, 6)), np.zeros((F, 6, 6)), np.zeros((F, 6, 6))
    for k in range(F):
        i, j = g["ij"][k]
        e, a, b = factor_jacobians(g["kinds"][k], poses[i], poses[j], g["data"][k])
        w = gps._whiten(g["kinds"][k], g["sigmas"][k])
        r[k], A[k], B[k] = e * w, a * w[:, None], b * w[:, None]
    return r, A, B


def norm2(g, poses, k):
    i, j = g["ij"][k]
    e = factor_residual(g["kinds"][k], poses[i], poses[j], g["data"][k])
    return float(np.sum((e * gps._whiten(g["kinds"][k], g["sigmas"][k])) ** 2))


def cost(g, poses):
    hub = robust.thresholds(g)
    s = 0.0
    for k in range(len(g["kinds"])):
        s += float(robust.term(hub[k], norm2(g, poses, k)))
    return s


def report(g, poses):
    hub = robust.thresholds(g)
    s2 = np.array([norm2(g, poses, k) for k in range(len(hub))])
    return (np.sqrt(s2), np.array([robust.weight(k, v) for k, v in zip(hub, s2)]).reshape(-1), np.array([robust.term(k, v) for k, v in zip(hub, s2)]).reshape(-1))


def linearize(g, poses):
    """whitened and weighted r, A, B at `poses`, and the weights [F]"""
    r, A, B = linearize_plain(g, poses)
    hub = robust.thresholds(g)
    w = np.ones(len(hub))
    for k in range(len(hub)):
        w[k] = robust.weight(hub[k], float(np.sum(r[k] ** 2)))
        if w[k] < 1.0:
            q = np.sqrt(w[k])
            r[k], A[k], B[k] = r[k] * q, A[k] * q, B[k] * q
    return r, A, B, w


def non_chain_edges(g):
    return gps.non_chain_edges(g)                       # (every kind but PRIOR counts there already)


def assemble(g, poses, sparse=False):
    n = len(poses)
    edges = [(int(i), int(j)) for i, j in g["ij"]]
    r, A, B, _ = linearize(g, poses)
    return (ref.assemble_sparse if sparse else ref.assemble)(n, g["fixed"], edges, r, A, B)


def gradient_norm(g, poses):
    return float(np.linalg.norm(assemble(g, poses)[1]))


def optimize(g, max_iterations=50, solver="direct"):
    """pose_graph_robust_ref.optimize's loop, line by line, with this module's cost and linearisation: (poses, stats)"""
    poses = np.array(g["poses"], np.float64)
    n, fixed = len(poses), g["fixed"]
    cap = 12 * non_chain_edges(g) + 64
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


# ---- graphs -----------------------------------------------------------------------------------------------------------------

def make_graph(poses, fixed, factors):
    """pose_graph_gps_ref.make_graph with a seventh entry per factor: (kind, i, j, data [16], sigmas [6], huber)"""
    g = gps.make_graph(poses, fixed, [f[:5] for f in factors])
    g["huber"] = np.array([f[5] for f in factors], np.float64)
    return g


def with_odom(drive, odom, T0, free, huber=ODOM_HUBER, which=None):
    """A drive of pose_graph_ref as a factor graph with the calibration node last, at T0: its BETWEEN factors, the calibration node's
    PRIOR of (0.5, 0.5, 1.5, 0.1, 0.1, 0.1) around T0 when `free` (held otherwise: the reference's prior of sigma 1e-6), then a
    HANDEYE of sigmas (0.2, 0.2, 0.2, 1.5, 1.5, 2) and threshold `huber` for every node in `which` (default: all), measured as odom[k]."""
    n = len(drive["poses"])
    which = range(n) if which is None else which
    factors = [(BETWEEN, int(i), int(j), gps.between_data(Z), ref.DEFAULT_SIGMAS, 0.0) for (i, j), Z in zip(drive["edges"], drive["Z"])]
    if free:
        factors.append((PRIOR, n, n, gps.prior_data(T0), CALIB_PRIOR_SIGMAS, 0.0))
    factors += [(HANDEYE, int(k), n, handeye_data(odom[k]), ODOM_SIGMAS, huber) for k in which]
    g = make_graph(list(drive["poses"]) + [T0], list(drive["fixed"]) + [0 if free else 1], factors)
    if "truth" in drive:
        g["truth"] = drive["truth"]
    return g
