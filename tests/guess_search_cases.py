"""Inputs shared by the guess-search tests (tests/guess_search_ref.py is the definition they are checked against)."""
import functools

import numpy as np

from staticmapping_amd import synth


@functools.lru_cache(maxsize=None)
def experiment():
    """The pair DESIGN.md §6 "Guess search" measures: two 20 000-point scans of synth.make_scene(0) taken 1.4 m and 5 degrees apart,
    and a guess that is off by (6.3, -4.2) m and 9 degrees -- 7.6 m of drift.  The target is taken at (10, -10) m, yaw 90 degrees, the
    scans with seeds 1 and 2.  Where the pair is taken matters, measured with the CPU oracle and the restatement: from the scene's origin
    the oracle's ICP still finds its way back from the drifted guess within its 150 iterations (0.35 m off with seeds 300 / 301, 0.002 m
    with 1 / 2); here it ends 1.17 m off with a score of 0.946, and the search puts it back.  At (5, 3) m, yaw 20 degrees, the drifted
    start ends 3.5 m off -- and the search itself peaks 1.2 m from the truth, along a wall, with a runner-up of 3 230 against 3 374: the
    case runner_up_score is reported for.  Returns (target [n, 4], source [n, 4], truth, guess)."""
    scene = synth.make_scene(0)
    pose_t = synth.make_pose(t=(10.0, -10.0, 0.0), rpy_deg=(0, 0, 90.0))
    pose_s = pose_t @ synth.make_pose(t=(0.0, 1.4, 0.0), rpy_deg=(0, 0, 5.0))
    target = synth.velodyne_scan(scene, pose_t, seed=1, n_points=20_000)
    source = synth.velodyne_scan(scene, pose_s, seed=2, n_points=20_000)
    truth = np.linalg.inv(pose_t) @ pose_s
    drift = synth.make_pose(t=(6.3, -4.2, 0.0), rpy_deg=(0, 0, 9.0))
    guess = truth.copy()
    guess[:3, :3] = drift[:3, :3] @ truth[:3, :3]
    guess[:3, 3] = truth[:3, 3] + drift[:3, 3]
    target.setflags(write=False)
    source.setflags(write=False)
    return target, source, truth, guess


def lattice(n, seed, res=0.5, span=12):
    """n distinct voxel centres (float32 rows [n, 4]) of a res-lattice within +-span voxels (z within +-2): exact in float32 for res
    a power of two"""
    rng = np.random.default_rng(seed)
    cells = set()
    while len(cells) < n:
        cells.add((int(rng.integers(-span, span)), int(rng.integers(-span, span)), int(rng.integers(-2, 3))))
    c = np.array(sorted(cells), np.float64)
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = (c + 0.5) * res
    return out
