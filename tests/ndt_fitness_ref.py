"""Brute-force reference for the per-query result of Ndt's fitness search (ndt_fit_near / ndt_fit_mid / ndt_fit_far behind
pcl::Registration::getFitnessScore).  numpy (and scipy's k-d tree for the scan cases) only; no grid of any kind in the lattice path.

Lattice cases.  Every coordinate is an integer number of units of 2^-6 m in [-512, 512) (so inside [-8, 8) m) and the pose is the
identity rotation with a translation of whole units.  The device's float transform 1 x + 0 y + 0 z + t and its distance
dx dx + dy dy + dz dz are then exact with or without FMA contraction: differences are k 2^-6 with |k| <= 2^10, squares k^2 2^-12 <= 2^20
units, a sum of three < 2^22 units < 2^24.  The reference is therefore integer arithmetic on the units, and a device distance must be
bit-equal to int_d2 / 4096 as float32.  `float32_brute_force` restates the float path on the host; test_ndt_fitness_ref.py holds it equal
to the integer one on every case.

Scan cases.  Arbitrary float32 clouds and poses: every query is moved in float64 by the float32 of the pose, d is its distance to the
nearest target point (k-d tree over the float64 target), and the device's squared distance may differ from d^2 by at most
    2 d E + E^2 + 8 2^-24 (d + E)^2,    E = |(E_x, E_y, E_z)|_2,   E_c = 3 2^-24 (|G_c0 x| + |G_c1 y| + |G_c2 z| + |G_c3|):
E_c bounds the three roundings of the float transform of coordinate c (each at most 2^-24 of a partial sum, which the sum of the
absolute addends bounds), the nearest-neighbour distance is 1-Lipschitz in the query, and the distance itself is eight float
operations.  Derived, not measured.

Stage rules (which pass may settle a query), from the kernels' own bounds with res the leaf size as a float and marg the table's margin:
    stage 0 => d <= res / 16;   stage 1 => d <= 0.875 res;   stage 2 => d > 0.75 res (1 - 1e-5) - marg res.
At leaf 1.0 a lattice query's fine cell is floor(units / 4) exactly, the fine cube is +-1 of it, and the first pass settles exactly the
queries whose best point inside the cube has int_d2 <= 15 (16 units^2 = (1/16 m)^2 is the bound itself and stays open; 15 is not a sum
of three squares, so on the lattice the largest settling value is 14).
"""
from __future__ import annotations

import math

import numpy as np

UNIT = 2.0 ** -6            # metres per lattice unit
BOX = 512                   # lattice coordinates lie in [-BOX, BOX)
FINE, MID, VOX = 4, 16, 64  # units per fine cell, mid cell and voxel at leaf 1.0
U24 = 2.0 ** -24
NO_SCORE = 1.7976931348623157e308      # what the search reports when no query is finite


def to_f32(units):
    """Lattice units -> float32 metres, rows x y z 0 (the layout the matchers upload)."""
    u = np.asarray(units, dtype=np.int64)
    out = np.zeros((len(u), 4), np.float32)
    out[:, :3] = (u * UNIT).astype(np.float32)
    return out


def int_brute_force(query_u, target_u, cube_fine=None):
    """For every query (moved, in units) the smallest integer squared distance to a target point -- all pairs, no grid.  With
    cube_fine = units per fine cell also the smallest over the targets whose fine cell is within +-1 of the query's on every axis
    (-1 where there is none)."""
    q = np.asarray(query_u, dtype=np.int32)
    t = np.asarray(target_u, dtype=np.int32)
    best = np.empty(len(q), np.int64)
    cube = np.full(len(q), -1, np.int64) if cube_fine else None
    step = max(1, (1 << 24) // max(1, len(t)))
    for a in range(0, len(q), step):
        qa = q[a:a + step]
        d = qa[:, None, :] - t[None, :, :]
        d2 = (d * d).sum(axis=2)
        best[a:a + step] = d2.min(axis=1)
        if cube_fine:
            fq = np.floor_divide(qa, cube_fine); ft = np.floor_divide(t, cube_fine)
            inside = (np.abs(fq[:, None, :] - ft[None, :, :]) <= 1).all(axis=2)
            m = np.where(inside, d2, np.iinfo(np.int32).max).min(axis=1).astype(np.int64)
            cube[a:a + step] = np.where(inside.any(axis=1), m, -1)
    return (best, cube) if cube_fine else best


def float32_brute_force(src_f32, target_f32, trans_f32):
    """The device's arithmetic on the host: float32 transform by the identity rotation and `trans`, float32 differences, squares
    and sums in the kernel's order, the minimum over all targets."""
    s = np.asarray(src_f32, np.float32)[:, :3]
    t = np.asarray(target_f32, np.float32)[:, :3]
    G = np.eye(3, dtype=np.float32)
    q = np.stack([((G[c, 0] * s[:, 0] + G[c, 1] * s[:, 1]) + G[c, 2] * s[:, 2]) + np.float32(trans_f32[c]) for c in range(3)], axis=1)
    assert q.dtype == np.float32
    best = np.empty(len(q), np.float32)
    step = max(1, (1 << 23) // max(1, len(t)))
    for a in range(0, len(q), step):
        d = t[None, :, :] - q[a:a + step, None, :]
        assert d.dtype == np.float32
        sq = d * d
        best[a:a + step] = ((sq[:, :, 0] + sq[:, :, 1]) + sq[:, :, 2]).min(axis=1)
    return best


def lattice_expected_d2(int_d2):
    """What the device must return, bit for bit."""
    return (np.asarray(int_d2, np.float64) / 4096.0).astype(np.float32)


def scan_reference(src_f32, target_f32, pose):
    """-> (d [ns] float64, tolerance [ns] on the squared distance) for a scan case."""
    from scipy.spatial import cKDTree
    G = np.asarray(pose, np.float64).astype(np.float32).astype(np.float64)      # the float matrix the device multiplies by
    s = np.asarray(src_f32, np.float32)[:, :3].astype(np.float64)
    moved = s @ G[:3, :3].T + G[:3, 3]
    d, _ = cKDTree(np.asarray(target_f32, np.float32)[:, :3].astype(np.float64)).query(moved)
    Ec = 3.0 * U24 * (np.abs(s) @ np.abs(G[:3, :3]).T + np.abs(G[:3, 3]))
    E = np.sqrt((Ec * Ec).sum(axis=1))
    tol = 2.0 * d * E + E * E + 8.0 * U24 * (d + E) ** 2
    return d, tol


def table_margin(target_f32, leaf):
    """The table's `marg` in cells (ndt_voxel_setup): 4 * 2^-24 * (largest |p * inv| of the target's box + 2)."""
    inv = np.float32(1.0) / np.float32(leaf)
    t = np.asarray(target_f32, np.float32)[:, :3]
    amax = max(float(np.abs(t.min(axis=0) * inv).max()), float(np.abs(t.max(axis=0) * inv).max()))
    return 4.0 * 5.9604645e-08 * (amax + 2.0)


def stage_violations(stage, d, leaf, marg):
    """Indices of the finite queries whose stage breaks a necessary condition.  d: reference distances in metres (float64)."""
    res = float(np.float32(leaf))
    stage = np.asarray(stage); d = np.asarray(d, np.float64)
    bad = ((stage == 0) & ~(d <= res / 16.0)) | ((stage == 1) & ~(d <= 0.875 * res)) | \
          ((stage == 2) & ~(d > 0.75 * res * (1.0 - 1e-5) - marg * res)) | (stage < 0) | (stage > 2)
    return np.nonzero(bad)[0]


def settles_in_the_fine_cube(cube_int_d2):
    """Leaf 1.0, lattice: the first pass settles a query exactly when its best point inside the fine cube has int_d2 <= 15."""
    c = np.asarray(cube_int_d2)
    return (c >= 0) & (c <= 15)


def score_of(d2_f32):
    """mean of the finite squared distances, summed exactly."""
    v = np.asarray(d2_f32, np.float32)
    f = v[np.isfinite(v)].astype(np.float64)
    return math.fsum(f.tolist()) / len(f) if len(f) else NO_SCORE
