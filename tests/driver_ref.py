"""The sequence driver's yardstick (a helper, not a test module): the synthetic drive written as KITTI `.bin` files, and the CPU
oracle's answer for every consecutive pair of such a directory -- computed from the FILES alone, so that nothing of the device
path (batched upload, Morton ordering, kd forest, slot parking, export, gather, chaining) has a hand in it.

Per pair k (scan k = target, scan k + 1 = source; builder/map_builder.cc:286, 302-333, 389):
  both files read back (`kitti.read_bin(f, scale_intensity=False)`), `cref.calculate_normals` on scan k's xyz as float64 in FILE
  order, rows with a non-finite normal dropped, then `cref.icp_fast_align(scan k + 1, q, n, guess)` with the driver's constant
  forward guess (`--guess-tx 0.6`).  `order=SEED` runs the same with scan k's rows under a seeded permutation: the kd-box
  subsampling of CalculateNormals is implementation-defined on tied coordinates (cloud_types.cc:347-368 sorts with std::sort),
  so a builder that starts from another row order may legally pick other leaves; tests/test_driver_ref.py bounds what that does
  to the pose.

The pose-file helpers print a chain the way the driver prints it (`ostream` with precision(8) = `%.8g` per entry, 12 per line,
builder/map_builder.cc:626-641), turn a chained file back into relative poses, and bound what the 8 significant digits cost."""
import os

import numpy as np

N_SCANS_FULL = 33                       # 32 pairs: one default batch of the driver
N_POINTS = 120_000
# the ragged set: scans 0-12 cut to these sizes (57344 = 7 * 2^13 and 57345 sit either side of the size where the kd tree gains
# a level: 8 192 and 8 193 leaves, as in tests/test_normals_exact_gpu.py); every batch of 5 mixes sizes
RAGGED_SIZES = (120000, 87001, 119999, 60000, 120000, 30011, 100003, 57345, 57344, 120000, 45000, 99999, 120000)
GUESS_TX = 0.6
ROT_TOL = 1e-4                          # rad, BASELINE.json north star: the tolerance of every oracle test of this project
TRANS_TOL = 1e-3                        # m
SCORE_TOL = 1e-4


def guess():
    G = np.eye(4)
    G[0, 3] = GUESS_TX
    return G


def drive_truth():
    """The generating poses of the full drive (tests/test_shard_driver_gpu.py::_drive's generator at 33 scans)."""
    from staticmapping_amd import synth
    return synth.drive_poses(N_SCANS_FULL, seed=5, speed=8.0, hz=10.0, yaw_rate_max=0.2)


def make_scans(n_scans=N_SCANS_FULL):
    """The first `n_scans` full-size scans of the 33-scan drive (the scene is always that of the whole drive, so scan k is the
    same cloud whatever n_scans is).  About 1.7 s of CPU per scan."""
    from staticmapping_amd import synth
    poses = drive_truth()
    scene = synth.make_drive_scene(poses, seed=5)
    return [synth.velodyne_scan(synth.scene_near(scene, P[:3, 3]), P, seed=1000 + k, n_points=N_POINTS) for k, P in enumerate(poses[:n_scans])]


def ragged_scan(scan, k):
    size = RAGGED_SIZES[k]
    if size == len(scan):
        return scan
    return scan[np.sort(np.random.default_rng(7000 + k).choice(N_POINTS, size, replace=False))]


def write_directory(directory, scans, ragged=False):
    """scans -> DIR/%010d.bin; ragged: scan k cut to RAGGED_SIZES[k] (at most 13 scans).  Returns the sorted file list."""
    from staticmapping_amd import kitti
    os.makedirs(directory, exist_ok=True)
    if ragged:
        scans = [ragged_scan(s, k) for k, s in enumerate(scans[:len(RAGGED_SIZES)])]
    for k, s in enumerate(scans):
        kitti.write_bin(kitti.scan_path(str(directory), k), s)
    return kitti.list_scans(str(directory))


class Oracle:
    """The oracle's rows for the pairs of one file set, each computed once per (pair, options)."""

    def __init__(self, files):
        self.files = list(files)
        self._rows = {}
        self._scan = {}

    def scan(self, k):
        """File k as the reader hands it on: float32 [N, 4]."""
        if k not in self._scan:
            from staticmapping_amd import kitti
            self._scan[k] = kitti.read_bin(self.files[k], scale_intensity=False)
        return self._scan[k]

    def xyz(self, k):
        return self.scan(k)[:, :3].astype(np.float64)

    def target(self, k, order=None):
        from oracle import cref
        p = self.xyz(k)
        if order is not None:
            p = p[np.random.default_rng(order).permutation(len(p))]
        q, n, _ = cref.calculate_normals(p)
        ok = np.isfinite(n).all(axis=1)
        return q[ok], n[ok]

    def pair(self, k, early_exit=False, max_iteration=None, order=None):
        """dict(result 4x4, score, iterations) of pair k: 20 fixed iterations, or early exit within 100."""
        if max_iteration is None:
            max_iteration = 100 if early_exit else 20
        key = (k, bool(early_exit), int(max_iteration), order)
        if key not in self._rows:
            q, n = self.target(k, order)
            self._rows[key] = self.icp(k, q, n, early_exit=early_exit, max_iteration=max_iteration)
        return self._rows[key]

    def icp(self, k, q, n, early_exit=False, max_iteration=None):
        """IcpFast alone: scan k + 1 against a target the caller hands in (the device's own prepared target, read back)."""
        from oracle import cref
        if max_iteration is None:
            max_iteration = 100 if early_exit else 20
        r = cref.icp_fast_align(self.xyz(k + 1), np.asarray(q, dtype=np.float64), np.asarray(n, dtype=np.float64), guess=guess(),
                                max_iteration=max_iteration, early_exit=bool(early_exit), nthreads=cref.usable_cores())
        return dict(result=r["result"], score=r["score"], iterations=r["iterations"])


_SETS = {}


def sequence_sets(tmp_path_factory):
    """The two directories the GPU modules run on -- the 33 full-size scans and the ragged 13 -- with an Oracle each.  Made once
    per test session (33 scans are about a minute of CPU, the oracle rows another half), whichever module asks first."""
    if not _SETS:
        scans = make_scans(N_SCANS_FULL)
        root = tmp_path_factory.mktemp("driver_sets")
        _SETS["full_dir"] = str(root / "full")
        _SETS["ragged_dir"] = str(root / "ragged")
        _SETS["full"] = Oracle(write_directory(_SETS["full_dir"], scans))
        _SETS["ragged"] = Oracle(write_directory(_SETS["ragged_dir"], scans, ragged=True))
    return _SETS


def se3_error(Ta, Tb):
    """(rotation angle of Ra Rb^T [rad], |ta - tb| [m]): BASELINE.json's metric, restated here so that the yardstick does not
    import the package under test for it."""
    R = Ta[:3, :3] @ Tb[:3, :3].T
    c = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
    s = np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2.0
    return float(np.arctan2(s, c)), float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3]))


# ---- kitti_pose.txt -------------------------------------------------------------------------------------------------------
def chain(rel):
    """pose_{k+1} = pose_k * T_k from the identity (builder/map_builder.cc:354)."""
    poses = [np.eye(4)]
    for T in rel:
        poses.append(poses[-1] @ np.asarray(T, dtype=np.float64))
    return np.stack(poses)


def write_chain(path, rel):
    """The chain of `rel` as the driver prints it: 12 entries per line, each as `%.8g`."""
    with open(path, "w") as f:
        for P in chain(rel):
            f.write(" ".join("%.8g" % v for v in P[:3, :].reshape(-1)) + "\n")


def read_chain(path):
    rows = np.loadtxt(path, dtype=np.float64, ndmin=2)
    assert rows.shape[1] == 12, rows.shape
    poses = np.tile(np.eye(4), (len(rows), 1, 1))
    poses[:, :3, :] = rows.reshape(-1, 3, 4)
    return poses


def relative_poses(poses):
    """inv(P_k) . P_{k+1} for a chained file's poses."""
    return np.stack([np.linalg.inv(poses[k]) @ poses[k + 1] for k in range(len(poses) - 1)])


def half_unit_8g(v):
    """The most `%.8g` can move v: half a unit of its 8th significant digit (0 prints exactly)."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    out = np.zeros_like(v)
    nz = v > 0
    out[nz] = 0.5 * 10.0 ** (np.floor(np.log10(v[nz])) - 7)
    return out


def file_precision_bound(poses):
    """(rad, m) that the relative poses of a chain can move by being printed with 8 significant digits and read back.

    Entry v moves by at most h(v) = half a unit of its 8th digit.  So the printed rotation block is R_k + E_k with
    |E_k|_F <= e_k = sqrt(sum h(R_ij)^2) and the printed translation t_k + d_k with |d_k| <= sqrt(sum h(t_i)^2).  To first order
      inv(R_k + E_k)(R_k+1 + E_k+1) - R_k^T R_k+1 = -R_k^T E_k R_k^T R_k+1 + R_k^T E_k+1,  Frobenius norm <= e_k + e_k+1,
    and se3_error's angle of (I + D) is at most |D|_F (its sine is half the norm of the antisymmetric part, <= |D|_F / sqrt 2).
      inv(R_k + E_k)(t_k+1 + d_k+1 - t_k - d_k) - R_k^T (t_k+1 - t_k):  norm <= |d_k| + |d_k+1| + e_k |t_k+1 - t_k|.
    The translation term grows with the chain's extent (h of a coordinate of 26 m is 5e-7 m), the rotation term does not.
    Second-order terms and the double arithmetic of the inverse are below 1e-13; the bound carries 1 % of slack for them."""
    poses = np.asarray(poses, dtype=np.float64)
    e = np.sqrt((half_unit_8g(poses[:, :3, :3]) ** 2).sum(axis=(1, 2)))
    d = np.sqrt((half_unit_8g(poses[:, :3, 3]) ** 2).sum(axis=1))
    step = np.linalg.norm(poses[1:, :3, 3] - poses[:-1, :3, 3], axis=1)
    rot = 1.01 * (e[:-1] + e[1:]).max()
    trans = 1.01 * (d[:-1] + d[1:] + e[:-1] * step).max()
    return float(rot), float(trans)
