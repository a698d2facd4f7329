"""The information of a point-to-plane alignment (include/smhip.h, smhip_icp_information) and the rule that turns it into a
pose-graph edge (include/smhip/edge_information.h), restated in numpy, f64.  The device kernel
(staticmapping_amd/csrc/smhip_icp_information.hip) and the header are tested against this file.

  matches     one FindClosests pass at T = (R, t), source -> target: brute force in f64, the first of equal distances
  kept        TrimmedDist(ratio): limit = the int(n * ratio)-th smallest of the n finite d2 (oracle/icp_fast.py's dists_quantile, with
              the ratio as the float32 option widened to double), kept = d2 finite and d2 <= limit
  row         m = R^T n,  r = n . (R s + t - q),  J = [s x m ; m]: the derivative of r under T <- T * [Exp(phi), rho] -- rotation
              first, the tangent of tests/pose_graph_ref.py's BETWEEN residual
  sums        H = sum J J^T,  sum_r2 = sum r^2 over the kept rows
"""
from __future__ import annotations

import numpy as np

from oracle import icp_fast as oracle_icp

DEFAULT_FLOOR = np.array([0.1, 0.1, 0.1, 0.15, 0.15, 0.15])


def brute_matches(moved, tgt, second=False):
    """ids [N], d2 [N] of the nearest target point of every moved source point (f64; a non-finite row: id -1, d2 inf); with
    `second`, also the runner-up's d2"""
    n = len(moved)
    ids, d2, d2b = np.full(n, -1, np.int64), np.full(n, np.inf), np.full(n, np.inf)
    ok = np.isfinite(moved).all(axis=1)
    for lo in range(0, n, 512):
        rows = np.nonzero(ok[lo:lo + 512])[0] + lo
        if len(rows) == 0:
            continue
        diff = moved[rows, None, :] - tgt[None, :, :]
        dd = np.einsum("ijk,ijk->ij", diff, diff)
        j = np.argmin(dd, axis=1)
        ids[rows], d2[rows] = j, dd[np.arange(len(rows)), j]
        if second and tgt.shape[0] > 1:
            dd[np.arange(len(rows)), j] = np.inf
            d2b[rows] = dd.min(axis=1)
    return (ids, d2, d2b) if second else (ids, d2)


def kept_set(d2, ratio):
    """(kept mask, limit_d2, n_finite) by the reference's quantile rule"""
    d2 = np.asarray(d2, np.float64)
    fin = np.isfinite(d2)
    if not fin.any():
        return np.zeros(len(d2), bool), 0.0, 0
    limit = oracle_icp.dists_quantile(np.where(fin, d2, np.inf), float(np.float32(ratio)))
    return fin & (d2 <= limit), limit, int(fin.sum())


def rows(src, q, n, R, t):
    """J [K, 6] and r [K] of source points src matched to target points q with normals n, at T = (R, t)"""
    m = n @ R                                        # rows R^T n
    J = np.concatenate([np.cross(src, m), m], axis=1)
    r = np.einsum("ij,ij->i", n, src @ R.T + t - q)
    return J, r


def information(src, tgt, nrm, T, ratio=0.7, ids=None, d2=None):
    """smhip_icp_information of (src, tgt with normals nrm) at T.  ids / d2: the matches to use (the device's own, so that both
    sides trim the same f32 distances); default: brute force."""
    src, tgt, nrm = np.asarray(src, np.float64), np.asarray(tgt, np.float64), np.asarray(nrm, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    if ids is None:
        ids, d2 = brute_matches(src @ R.T + t, tgt)
    keep, limit, n_finite = kept_set(d2, ratio)
    k = np.nonzero(keep)[0]
    J, r = rows(src[k], tgt[ids[k]], nrm[ids[k]], R, t)
    return dict(H=J.T @ J, sum_r2=float(r @ r), kept=int(len(k)), n_finite=n_finite, limit_d2=float(limit), rows=k, J=J, r=r, ids=ids)


def edge_information(H, sum_r2, kept, floor=DEFAULT_FLOOR, min_residual_sigma=0.02, information_scale=1.0, max_inflation=100.0):
    """MakeEdgeInformation with numpy's eigh: dict(L, strength, weakest, residual_sigma)"""
    floor = np.asarray(floor, np.float64)
    sigma2 = min_residual_sigma ** 2
    Hw = np.zeros((6, 6))
    if kept > 6:
        sigma2 = max(sum_r2 / (kept - 6), sigma2)
        Hw = information_scale * 0.5 * (H + H.T) / sigma2 * np.outer(floor, floor)
    h, Q = np.linalg.eigh(Hw)
    h = np.maximum(h, 0.0)
    g = np.maximum(h / (1.0 + h), 1.0 / max_inflation ** 2)
    L = np.sqrt(g)[:, None] * Q.T / floor[None, :]
    w = Q[:, 0] * floor
    w = w / np.linalg.norm(w)
    if w[int(np.argmax(np.abs(w)))] < 0.0:
        w = -w
    return dict(L=L, strength=h, weakest=w, residual_sigma=float(np.sqrt(sigma2)))


# ---- fixtures: surfaces with analytic normals, a source drawn on the same surfaces, moved by the inverse of a known pose --------
def _pose(rpy_deg, t):
    from staticmapping_amd import synth
    return synth.make_pose(t=t, rpy_deg=rpy_deg)


def _sample(rng, n, faces):
    """n points spread over `faces` = [(origin, edge u, edge v, normal)], with the faces' normals"""
    p, nn = np.zeros((n, 3)), np.zeros((n, 3))
    which = np.arange(n) % len(faces)
    uv = rng.uniform(0.0, 1.0, size=(n, 2))
    for f, (o, u, v, nrm) in enumerate(faces):
        k = which == f
        p[k] = np.asarray(o) + uv[k, :1] * np.asarray(u) + uv[k, 1:] * np.asarray(v)
        nn[k] = nrm
    return p, nn


PLANE = [((0, 0, 0), (6, 0, 0), (0, 6, 0), (0, 0, 1))]
CORRIDOR = [((0, -1.5, 0), (12, 0, 0), (0, 0, 2.5), (0, 1, 0)),          # left wall
            ((0, 1.5, 0), (12, 0, 0), (0, 0, 2.5), (0, -1, 0)),          # right wall
            ((0, -1.5, 0), (12, 0, 0), (0, 3, 0), (0, 0, 1))]            # floor: nothing constrains x


def surface_pair(faces, n_src, n_tgt, seed, sigma=0.005, rpy_deg=(1.0, -2.0, 3.0), t=(0.30, -0.20, 0.10)):
    """(src [n_src, 4] f32 in its own frame, tgt [n_tgt, 3] f64-of-f32, normals [n_tgt, 3] f64-of-f32, T source -> target)"""
    rng = np.random.default_rng(seed)
    tgt, nrm = _sample(rng, n_tgt, faces)
    s_in_t, _ = _sample(rng, n_src, faces)
    s_in_t = s_in_t + rng.normal(0.0, sigma, size=s_in_t.shape)
    T = _pose(rpy_deg, t)
    Ti = np.linalg.inv(T)
    src = np.zeros((n_src, 4), np.float32)
    src[:, :3] = (s_in_t @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    return src, tgt.astype(np.float32).astype(np.float64), nrm.astype(np.float32).astype(np.float64), T
