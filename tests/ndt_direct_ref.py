"""pclomp's direct voxel neighbourhoods (setNeighborhoodSearchMethod DIRECT26 / DIRECT7 / DIRECT1) on the CPU, written from the
rule of pclomp/voxel_grid_covariance_omp_impl.hpp:373-442 as a dictionary look-up.  numpy, oracle.ndt and ndt_deriv_ref only.

The rule.  The centre cell of a transformed point x (float) is floor(x / leaf) per axis, a float DIVISION (:379-381; the voxel
build multiplies by the inverse leaf size instead, :218-220).  A cell of the mode's stencil is kept when it lies inside the
target's voxel box on every axis (:382-392), is occupied and holds min_points_per_voxel points (:395).  No distance enters.
  DIRECT1   the centre cell                                  (:438-442)
  DIRECT7   the centre cell and its six face neighbours      (:419-433)
  DIRECT26  the 26 cells around the centre WITHOUT the centre: pcl::getAllNeighborCellIndices() of PCL 1.8.1 (13 half-neighbours
            and their negatives).  PCL is not vendored by the reference: this stencil is unpinned like the other registrator oracles.
A row that is not finite has no pairs.
"""
from __future__ import annotations

import functools

import numpy as np

import ndt_deriv_ref as R
from oracle import ndt as ondt

F = np.float32
KDTREE, DIRECT26, DIRECT7, DIRECT1 = 0, 1, 2, 3          # pclomp/ndt_omp.h:52-57
DIRECT_MODES = (DIRECT26, DIRECT7, DIRECT1)
MODE_NAMES = {KDTREE: "KDTREE", DIRECT26: "DIRECT26", DIRECT7: "DIRECT7", DIRECT1: "DIRECT1"}

# ndt_deriv_ref's tolerance rule on the direct pair sets: RHO = the largest |oracle - reference| / S_c over its cases, the three
# modes and both arithmetics, measured by `python -m pytest tests/test_ndt_direct_ref.py -q -s -k measured` (which asserts that
# RHO still bounds what it measures); K = 4 max(1, RHO) rounded up to a power of two.  It is larger than ndt_deriv_ref.RHO
# (0.7394): DIRECT1 on the one-point source (block/ns1/Pc, gradient component 4) sums ONE pair, so the float rounding of the
# oracle's single evaluation stands against the S_c of a single addend with nothing to average it.
RHO = 1.5499
K = 8.0


def stencil(mode):
    """The relative cells (dx, dy, dz) of a mode, in z, y, x order."""
    cells = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    if mode == DIRECT26:
        return [c for c in cells if c != (0, 0, 0)]
    if mode == DIRECT7:
        return [c for c in cells if abs(c[0]) + abs(c[1]) + abs(c[2]) <= 1]
    if mode == DIRECT1:
        return [(0, 0, 0)]
    raise ValueError(f"not a direct mode: {mode}")


def centre_cells(xt, leaf):
    """floor(x / leaf) in float, per axis, as integers (rows that are not finite: zeros, see `finite`)."""
    x = np.asarray(xt, dtype=F)
    ok = np.isfinite(x).all(axis=1)
    q = np.where(ok[:, None], x, F(0)) / F(leaf)            # float32 / float32: the correctly rounded quotient
    assert q.dtype == F
    return np.floor(q).astype(np.int64), ok


def _kept_voxels(table_or_grid):
    """{linear key: voxel index} of the voxels a direct rule may return: occupied and with min_points.  An ndt_deriv_ref.Table
    lists every occupied voxel (the index is the device's slot); an oracle VoxelGrid holds the searchable ones only."""
    t = table_or_grid
    keys = np.asarray(t.key).tolist()
    if hasattr(t, "n"):
        keep = t.searchable()
        return {k: v for v, k in enumerate(keys) if keep[v]}
    return {k: v for v, k in enumerate(keys)}


def direct_pairs(table_or_grid, xt, mode, leaf=1.0):
    """(point index, voxel index) of every pair the mode returns, by point, then in the stencil's z, y, x order."""
    t = table_or_grid
    kept = _kept_voxels(t)
    min_b = np.asarray(t.min_b, dtype=np.int64); div_b = np.asarray(t.div_b, dtype=np.int64)
    max_b = min_b + div_b - 1
    c, ok = centre_cells(xt, leaf)
    look = np.vectorize(lambda k: kept.get(k, -1), otypes=[np.int64])
    pi, vi, rank = [], [], []
    for s, d in enumerate(stencil(mode)):                    # a stencil cell for all points at once
        ijk = c + np.asarray(d)
        inside = ok & (ijk >= min_b).all(axis=1) & (ijk <= max_b).all(axis=1)            # :392
        r = ijk[inside] - min_b
        v = look(r[:, 0] + r[:, 1] * div_b[0] + r[:, 2] * div_b[0] * div_b[1]) if inside.any() else np.zeros(0, np.int64)   # :394-395
        found = v >= 0
        pi.append(np.nonzero(inside)[0][found]); vi.append(v[found]); rank.append(np.full(int(found.sum()), s))
    pi, vi, rank = np.concatenate(pi), np.concatenate(vi), np.concatenate(rank)
    order = np.lexsort((rank, pi))
    return pi[order].astype(np.int64), vi[order].astype(np.int64)


def brute_force_count(table: R.Table, xt, mode, leaf=1.0):
    """The number of pairs by looking at EVERY voxel of the table for every point (no dictionary, no box test: a voxel of the
    table is inside the box)."""
    c, ok = centre_cells(xt, leaf)
    keep = table.searchable()
    cell = (table.idx + table.min_b)[keep]                   # absolute cell of each kept voxel
    disp = cell[None, :, :] - c[:, None, :]                  # [points, voxels, 3]
    st = np.asarray(stencil(mode))
    hit = (disp[:, :, None, :] == st[None, None, :, :]).all(axis=3).any(axis=2)
    return int(hit[ok].sum())


class DirectVoxelGrid(ondt.VoxelGrid):
    """oracle.ndt.VoxelGrid whose neighbourhoods are a direct mode's: compute_derivatives and ndt_align take theirs from
    radius_pairs, so this gives the oracle's whole alignment in that mode."""

    def __init__(self, target_f32, mode, resolution: float = 1.0, **kw):
        super().__init__(target_f32, resolution, **kw)
        self.mode = mode

    def radius_pairs(self, x_trans_f32):
        return direct_pairs(self, x_trans_f32, self.mode, self.resolution)


def reference(table, src, xt, pose, d1, d2, double_math, hessian, mode, leaf=1.0) -> R.Reference:
    """ndt_deriv_ref.reference with the mode's pair set: values, A, the ulp-move spread N (pair set frozen) and S = u A + N."""
    pairs = direct_pairs(table, xt, mode, leaf)
    vals, A, npairs, pairs, e = R.evaluate(table, src, xt, pose, d1, d2, double_math, hessian, pairs=pairs)
    N = np.zeros(28)
    for t in range(16):
        moved, _, _, _, _ = R.evaluate(table, src, R._ulp_moves(xt, 7000 + t), pose, d1, d2, double_math, hessian, pairs=pairs)
        N = np.maximum(N, np.abs(moved - vals))
    u = 2.0 ** -53 if double_math else 2.0 ** -24
    return R.Reference(vals, A, N, u * A + N, npairs, pairs, e)


@functools.lru_cache(maxsize=None)
def case_reference(name, d1, d2, double_math, hessian, mode) -> R.Reference:
    c = R.case(name)
    return reference(R.tables()[c.target], c.src, R.case_xt(c), c.pose, d1, d2, double_math, hessian, mode)


# ---------------------------------------------------------------------------------------------
# division against multiplication by the inverse, at a leaf that is no power of two
# ---------------------------------------------------------------------------------------------
LEAF_03 = 0.3


@functools.lru_cache(maxsize=None)
def disagreeing_floats(leaf=LEAF_03):
    """Of the floats k * leaf (float product) and their two float neighbours, k in -400 .. 399, those whose cell by division,
    floor(x / leaf), is not their cell by the build's multiplication, floor(x * (1 / leaf)): (x, cell by division, cell by
    multiplication), all float32 arithmetic."""
    lf = F(leaf)
    inv = F(1.0) / lf
    k = np.arange(-400, 400).astype(F)
    x0 = (k * lf).astype(F)
    x = np.concatenate([np.nextafter(x0, F(-np.inf)), x0, np.nextafter(x0, F(np.inf))]).astype(F)
    cd = np.floor((x / lf).astype(F)).astype(np.int64)
    cm = np.floor((x * inv).astype(F)).astype(np.int64)
    bad = cd != cm
    return x[bad], cd[bad], cm[bad]


@functools.lru_cache(maxsize=None)
def division_case(nq=24):
    """A target at resolution 0.3 and queries on which the two cell rules disagree.  Query j sits in a (y, z) row of its own, at an
    x where floor(x / leaf) != floor(x * inv); the two cells on either side of that x are both occupied, one with 8 points and
    the other with 5 (below min_points): for even j the division's cell is the searchable one, for odd j the multiplication's.
    So DIRECT1 by the division rule pairs exactly the even queries, and by the multiplication rule exactly the odd ones.  The
    pose is ndt_deriv_ref's exact one (identity rotation, dyadic translation); only queries whose float transform returns x
    itself are used.  Target points are lattice points well inside their cells, where both rules agree.
    Returns dict(target [nt, 4] f32, src [nq, 4] f32, xt [nq, 3] f32, pose, expect_div (bool per query), expect_mul)."""
    lf = F(LEAF_03)
    pose = np.array(R.POSES["Pi"])
    t = pose[:3].astype(F)
    xs, cd, cm = disagreeing_floats()
    sx = (xs - t[0]).astype(F)
    exact = (sx + t[0]).astype(F) == xs
    # spread over the scanned range, one query per x
    pick = np.nonzero(exact)[0]
    pick = pick[np.linspace(0, len(pick) - 1, nq).round().astype(int)]
    assert len(set(pick.tolist())) == nq
    rng = np.random.default_rng(303)
    tgt, src = [], []
    expect_div = np.zeros(nq, dtype=bool)
    for j, q in enumerate(pick):
        cy, cz = 2 * j, 0                                    # the row's cell; rows two cells apart
        y = F((cy + 0.5) * float(lf)); z = F((cz + 0.5) * float(lf))
        sy = F(y - t[1]); sz = F(z - t[2])
        src.append([sx[q], sy, sz, 0.0])
        searchable_cell, sparse_cell = (cd[q], cm[q]) if j % 2 == 0 else (cm[q], cd[q])
        expect_div[j] = j % 2 == 0
        for cell, n in ((searchable_cell, 8), (sparse_cell, 5)):
            lo = np.array([cell, cy, cz]) * float(lf)
            f = rng.uniform(0.25, 0.75, (n, 3)) * float(lf)
            tgt.append(np.round((lo + f) * 1024) / 1024)     # 2^-10 lattice: a voxel's sums are exact
    tgt = np.concatenate(tgt)
    tgt = np.concatenate([tgt, np.zeros((len(tgt), 1))], axis=1).astype(F)
    src = np.asarray(src, dtype=F)
    xt = R.transform_f32(src, R.pose_matrix_f32(pose))
    assert (xt[:, 0] == xs[pick]).all()
    return dict(target=tgt, src=src, xt=xt, pose=pose, expect_div=expect_div, expect_mul=~expect_div, cd=cd[pick], cm=cm[pick])


# ---------------------------------------------------------------------------------------------
# whole alignments
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden_pair():
    """The pair of tests/golden/make_golden.py::ndt_case: two 8 000-point scans merged as the target, the third as the source,
    the guess 0.25 m short."""
    from staticmapping_amd import synth
    scene = synth.make_scene(0)
    poses = [synth.make_pose(t=(0.8 * k, 0.0, 0.0)) for k in range(3)]
    scans = [synth.velodyne_scan(scene, P, seed=20 + k, n_points=8000) for k, P in enumerate(poses)]
    tgt = np.concatenate([s[:, :3].astype(np.float64) @ P[:3, :3].T + P[:3, 3] for s, P in zip(scans[:2], poses[:2])]).astype(F)
    G = poses[2].copy(); G[0, 3] -= 0.25
    return scans[2], tgt, G, poses[2]


# guesses of the batch test: the golden guess moved in x and y and turned about z; chosen on the CPU so that the oracle's DIRECT7
# alignments take 2, 3, 4 and 3 iterations (test_ndt_direct_ref.py asserts that they are not all equal)
BATCH_OFFSETS = ((0.0, 0.0, 0.0), (0.25, 0.2, 1.0), (0.0, 0.3, 0.0), (0.1, -0.2, 3.0))       # (metres along x, y; degrees about z)


def batch_guesses():
    from staticmapping_amd import synth
    _, _, G, _ = golden_pair()
    return [G @ synth.make_pose(t=(dx, dy, 0.0), rpy_deg=(0, 0, yaw)) for dx, dy, yaw in BATCH_OFFSETS]


@functools.lru_cache(maxsize=None)
def oracle_align(mode, guess_index=None):
    """oracle.ndt.ndt_align on the golden pair in `mode` (KDTREE: the oracle's own grid), from the golden guess or batch guess k."""
    src, tgt, G, _ = golden_pair()
    if guess_index is not None:
        G = batch_guesses()[guess_index]
    grid = ondt.VoxelGrid(tgt) if mode == KDTREE else DirectVoxelGrid(tgt, mode)
    return ondt.ndt_align(src, tgt, guess=G, grid=grid)
