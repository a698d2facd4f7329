"""numpy restatement of "motion compensation after optimisation" (a helper, not a test module).

Sweep motions, from the frame poses P_0 .. P_{n-1} of the whole run (as written to the pose file and parsed back):

    delta_k     = RigidInverse(P_k) P_{k+1}     k < n - 1
    delta_{n-1} = delta_{n-2};  n == 1: the identity

with RigidInverse = (R^T, -R^T t) as in include/smhip/front_end.h.  Which frames a map inserts does not change the two poses that
define a frame's motion.  Products and sums are written in the order include/smhip/sweep_motion.h evaluates them, in Python floats,
so the doubles are the same ones.

Compensated row i of a frame of n rows: its factor f_i is float32(float64(i) / float64(n)) for 4-float rows (the collector's rule)
and row[4] for 5-float rows.  Then, in this order,
  1. MotionCompensation(row, delta_k) as tests/motion_comp_ref.py restates it (double, each coordinate cast to float; intensity and
     factor carried),
  2. the float TransformPoint under P_k (tests/test_static_map_gpu.py::oracle_rows), intensity times intensity_scale.
The ray origin stays the float translation of P_k: the pose is the sensor pose at the start of the frame's sweep."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_comp_ref as mc  # noqa: E402
from icp_compensation_ref import skew  # noqa: E402,F401  (the drive's skewed scans)
from test_static_map_gpu import oracle_rows  # noqa: E402


def rigid_inverse(P):
    t = [[float(P[r][c]) for c in range(4)] for r in range(4)]
    out = np.eye(4)
    for i in range(3):
        for j in range(3):
            out[i, j] = t[j][i]
    for i in range(3):
        out[i, 3] = -(float(out[i, 0]) * t[0][3] + float(out[i, 1]) * t[1][3] + float(out[i, 2]) * t[2][3])
    return out


def multiply(A, B):
    out = np.zeros((4, 4))
    for r in range(4):
        for c in range(4):
            s = 0.0
            for k in range(4):
                s += float(A[r][k]) * float(B[k][c])
            out[r, c] = s
    return out


def sweep_motions(poses):
    """[n, 4, 4] float64: the sensor's motion during every frame's sweep."""
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    n = len(poses)
    out = np.tile(np.eye(4), (n, 1, 1))
    for k in range(n - 1):
        out[k] = multiply(rigid_inverse(poses[k]), poses[k + 1])
    if n >= 2:
        out[n - 1] = out[n - 2]
    return out


def factors(rows):
    """f_i of every row: float32 [n]."""
    rows = np.asarray(rows, np.float32)
    n = len(rows)
    if rows.shape[1] > 4:
        return rows[:, 4].copy()
    return (np.arange(n, dtype=np.float64) / np.float64(n)).astype(np.float32)


def deskewed_rows(rows, motion):
    """Step 1: [n, 5] float32 rows x y z intensity factor in the frame of the sweep's start."""
    rows = np.asarray(rows, np.float32)
    rows5 = np.concatenate([rows[:, :4], factors(rows)[:, None]], axis=1).astype(np.float32)
    return mc.motion_compensation(rows5, motion)


def compensated_world_rows(rows, pose, motion, intensity_scale=1.0):
    """Steps 1 and 2: the [n, 5] float32 rows the map takes in."""
    return oracle_rows(deskewed_rows(rows, motion), pose, intensity_scale)


def skewed_drive(n_scans=4, n_points=5_000, seed=5):
    """The drive of the checks: dict(poses [n, 4, 4], motions, clean = the scans as a sensor at rest at each pose sees them,
    skewed = the same scans as taken during the motion to the next pose)."""
    from staticmapping_amd import synth
    poses = synth.drive_poses(n_scans, seed=seed, speed=8.0, hz=10.0, yaw_rate_max=0.2)
    scene = synth.make_drive_scene(poses, seed=seed)
    clean = [synth.velodyne_scan(synth.scene_near(scene, P[:3, 3]), P, seed=1000 + k, n_points=n_points)[:, :4] for k, P in enumerate(poses)]
    motions = sweep_motions(poses)
    return dict(poses=np.asarray(poses), motions=motions, clean=clean, skewed=[skew(s, d) for s, d in zip(clean, motions)])


def kept_keys(ora, threshold=0.6):
    """The voxels an oracle map's output keeps, as a set of (x, y, z)."""
    keys, prob, _, npts, _ = ora.dump()
    keep = (prob >= int(np.float32(threshold) * np.float32(256))) & (npts > 0)
    return set(map(tuple, keys[keep].tolist()))


def differing_share(a, b):
    """Keys in one set and not in the other, relative to |a|."""
    return len(a ^ b) / float(len(a))
