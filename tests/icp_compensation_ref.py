"""numpy float64 restatement of IcpFast with INNER MOTION COMPENSATION (a helper, not a test module).

The reference's branch (registrators/icp_fast.cc:486-491 -> builder/data/cloud_types.cc:306-321) is undefined behaviour as
written: `ApplyMotionCompensation` declares a local `transform` inside its own initialiser.  Its intent is plain from three places:

    icp_fast.cc:486-491      the step cloud is init_source with point i moved by InterpolateTransform(I, T_iter, factor_i)
    icp_fast.cc:130, 284-289 the columns of F and wF are scaled by factor_i
    cloud_types.cc:340-343   factor_i = i / size

THIS FILE IS THE DEFINITION the library implements (smhip_icp_set_inner_compensation); the reference is its source where the
reference is defined.  Built on oracle.icp_fast's functions and tests/motion_comp_ref.py; compared with `icp_fast_align` only two
things differ:

  1. the step cloud.  P0 = T(-mu) guess s_i as in the rigid Align; with n rows (NaN rows included) and i the caller's row index,
     f_i = (double) i / n; the interpolation sees (double)(float) f_i (common::InterpolateTransform takes a const float):
         P_i = R(f_i) P0_i + T_iter.t * f_i,   R = motion_comp_ref.interpolated_rotations(T_iter, f)
     and EACH COORDINATE IS ROUNDED TO FLOAT and widened again: the step cloud is a float cloud.
  2. the sums.  With J_i = [P_i x n ; n], r_i = (P_i - q) . n over the kept i:
         A = sum f_i^2 J_i J_i^T,   b = -sum f_i J_i r_i        f_i the unrounded double i / n

Search, quantile rank rule, `<=`, solve, the NaN -> identity rule, T_iter = dT T_iter, history, CheckConvergence, the score of the
last iteration's kept matches and result = T(mu) T_iter T(-mu) guess are unchanged.  The guess is the pose at the start of the
sweep, the motion during the sweep the unknown, the result the pose at its end."""
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_comp_ref as mc  # noqa: E402
from oracle import icp_fast as ref  # noqa: E402


def factors(n, rows=None):
    """f_i = (double) i / n for the caller's row indices `rows` (default: 0 .. n-1)."""
    i = np.arange(n, dtype=np.float64) if rows is None else np.asarray(rows, dtype=np.float64)
    return i / float(n)


def step_cloud(P0, T_iter, f):
    """The compensated step cloud as the float cloud it is: [N, 3] float64 holding float32 values."""
    f32 = np.asarray(f, np.float64).astype(np.float32)
    t = f32.astype(np.float64)
    R = mc.interpolated_rotations(T_iter, f32)
    x, y, z = P0[:, 0], P0[:, 1], P0[:, 2]
    out = np.empty_like(P0)
    with np.errstate(invalid="ignore"):
        for r in range(3):
            out[:, r] = ((R[:, r, 0] * x + R[:, r, 1] * y) + R[:, r, 2] * z) + T_iter[r, 3] * t
        return out.astype(np.float32).astype(np.float64)


def compute_point_to_plane(reading, ref_pts, ref_nrm, f):
    """oracle.icp_fast.compute_point_to_plane with the columns of F scaled by the factor (icp_fast.cc:284-289)."""
    cross = np.cross(reading, ref_nrm)
    F = np.concatenate([cross, ref_nrm], axis=1) * np.asarray(f, np.float64)[:, None]
    A = F.T @ F
    dot = np.einsum("ij,ij->i", reading - ref_pts, ref_nrm)
    b = -(F.T @ dot)
    x = ref.solve_possibly_underdetermined(A, b)
    T = np.eye(4)
    T[:3, :3] = ref.angle_axis_matrix(x[:3])
    T[:3, 3] = x[3:6]
    if np.isnan(T).any():
        T[:3, :3] = np.eye(3)
    return T, A, b


def icp_fast_align_compensated(source, target, target_normals, guess=None, max_iteration=100, dist_outlier_ratio=0.7,
                               early_exit=True, rows=None, trace=None):
    """IcpFast::Align with inner compensation.  `rows`: the caller's row index of every source row (default: its position).
    Source rows with a NaN coordinate take no part in the search (the device gives them no match) but count in n.
    Returns (result 4x4, score, iterations)."""
    S = np.asarray(source, dtype=np.float64)
    Q = np.asarray(target, dtype=np.float64)
    Nrm = np.asarray(target_normals, dtype=np.float64)
    if guess is None:
        guess = np.eye(4)
    n = S.shape[0]
    f_all = factors(n, rows)
    good = np.isfinite(S).all(axis=1)
    S, f = S[good], f_all[good]
    rho = float(np.float32(dist_outlier_ratio))
    mu = Q.sum(axis=0) / Q.shape[0]
    T_mean = np.eye(4); T_mean[:3, 3] = mu
    Qc = Q - mu
    tree = cKDTree(Qc)
    T_mean_inv = np.eye(4); T_mean_inv[:3, 3] = -mu
    G = T_mean_inv @ guess
    P0 = ref.apply_transform(S, G)
    T_iter = np.eye(4)
    rots = [np.array([1.0, 0, 0, 0])]
    trans = [np.zeros(3)]
    it = 0
    while True:
        P = step_cloud(P0, T_iter, f)
        ids, d2 = ref.find_closests(tree, Qc, P)
        limit = ref.dists_quantile(d2, rho)
        keep = (d2 <= limit) & (d2 != np.inf)
        dT, A, b = compute_point_to_plane(P[keep], Qc[ids[keep]], Nrm[ids[keep]], f[keep])
        if trace is not None:
            trace.append(dict(ids=ids, d2=d2, limit=limit, keep=keep, A=A, b=b, T_before=T_iter.copy(), dT=dT, good=good, P=P))
        T_iter = dT @ T_iter
        it += 1
        rots.append(ref._quat_from_matrix(T_iter[:3, :3]))
        trans.append(T_iter[:3, 3].copy())
        if (early_exit and ref.check_convergence(rots, trans)) or it >= max_iteration:
            score = float(np.exp(-np.sqrt(d2[keep]).sum() / keep.sum()))
            break
    return T_mean @ T_iter @ G, score, it


def prototype_case(n_points=20_000):
    """The experiment of DESIGN.md section 6: a scan taken during a motion, aligned from the pose at the start of its sweep.
    Returns dict(src_skewed [N, 3] f64, q, n, start, end)."""
    from staticmapping_amd import synth
    scene = synth.make_scene(0)
    tgt = synth.velodyne_scan(scene, synth.make_pose(), seed=2, n_points=n_points)
    q, nrm, _ = ref.calculate_normals(tgt[:, :3].astype(np.float64))
    ok = np.isfinite(nrm).all(axis=1)
    start = synth.make_pose(t=(0.5, 0.02, 0.0), rpy_deg=(0.0, 0.0, 0.8))
    src = synth.velodyne_scan(scene, start, seed=3, n_points=n_points)
    delta = synth.make_pose(t=(0.80, 0.05, 0.01), rpy_deg=(0.2, 0.2, 1.5))
    skewed = skew(src, delta)
    return dict(src_skewed=skewed[:, :3].astype(np.float64), q=q[ok], n=nrm[ok], start=start, delta=delta, end=delta @ start)


def skew(rows4, delta):
    """The rows whose compensation under `delta` gives rows4 back (tests/test_front_end_mc_gpu.py's _skew): p' = R(f)^-1 (p - t f)."""
    rows4 = np.asarray(rows4, np.float32)
    f32 = (np.arange(len(rows4), dtype=np.float64) / len(rows4)).astype(np.float32)
    f = f32.astype(np.float64)
    R = mc.interpolated_rotations(delta, f32)
    p = rows4[:, :3].astype(np.float64) - np.outer(f, delta[:3, 3])
    out = rows4.copy()
    out[:, :3] = np.linalg.solve(R, p[:, :, None])[:, :, 0].astype(np.float32)
    return out
