"""Constructed inputs and a float64 reference for ONE computeDerivatives evaluation of registrators::Ndt
(pclomp/ndt_omp_impl.hpp:180-284, 397-438, 483-535) and for the voxel table under it
(pclomp/voxel_grid_covariance_omp_impl.hpp:49-370).  CPU only: numpy and oracle.ndt's constants and angle tables, nothing of the device.

Coordinates.  Every target point lies on a binary lattice (2^-10 m; 2^-8 m in the crowded voxels) with
n * max|x| / quantum < 2^24 in every voxel, so a voxel's float centroid sums and its double mean / product sums are exact in
any order: a wave-parallel sum and a sequential one give the same bits, the centroid and the mean have one value, and the radius
test |x_trans - centroid|^2 <= res^2 is decided from identical centroids everywhere.  `check_lattice` asserts that.

Margins.  After the float transform no query coordinate is within MARGIN of a lattice plane (except the queries put on planes on
purpose, which use a pose whose float transform is exact) and no candidate pair's centroid distance is within MARGIN of the
resolution: the set of (point, voxel) pairs does not depend on a last-bit difference of the transform.  Seeds are searched until
both hold.  The margins are conditions on the inputs -- no pair is ever excused.

Tolerance.  For every component c (score, 6 gradient, 21 Hessian) the reference also returns
  A_c  the sum over the pairs of the absolute values of the component's addends (a Hessian entry has three per pair:
       -d2 (x'CJ_i)(x'CJ_j), x'C H_ij, J_j C J_i, each times e), and
  N_c  the largest change of the component over 16 seeded re-evaluations with every transformed coordinate moved by -1, 0 or +1
       float ulp and the pair set frozen (a device may contract the transform into FMAs: its x_trans is known to an ulp only).
The scale is S_c = u A_c + N_c, u = 2^-24 for the float path and 2^-53 for the double path, and a device is allowed K S_c.  K is
not chosen: RHO below is the largest |oracle_c - ref_c| / S_c over all cases and components, the oracle being
oracle/ndt.py::compute_derivatives -- pclomp's own per-pair float association (real=None) and stock PCL's double one
(real=np.float64) -- and K = 4 max(1, RHO) rounded up to a power of two.  The factor 4 is for what a device legitimately does
differently from the oracle: a point's terms summed in R before the Jacobian algebra, its own expf / exp, FMA contraction.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from oracle import ndt as ondt

F = np.float32
MARGIN = 1e-4
Q10, Q8 = 2.0 ** -10, 2.0 ** -8
MIN_POINTS, EIG_MULT, RESOLUTION = 6, 0.01, 1.0
BIG_VOXEL = 2048            # kNdtBigVoxel: voxels with MORE points are summed by ndt_voxel_stats_big
PAIR_CAP = 1024             # kNdtPairCap: list entries per wave and window
MAX_WORDS = 1 << 20         # kNdtMaxWords

# measured by `python -m pytest tests/test_ndt_deriv_ref.py -q -s -k measured` (it prints both and asserts RHO still bounds what
# it measures); K = 4 * max(1, RHO) rounded up to a power of two
RHO = 0.7394
K = 4.0

POSES = {
    "Pa": (0.11, -0.07, 0.05, 0.02, -0.03, 0.04),
    "Pb": (-0.08, 0.06, 0.09, 0.3, -0.2, 0.5),           # every row of h_ang carries weight
    "Pc": (0.05, 0.04, -0.06, 5e-5, 5e-5, 5e-5),         # small-angle rule: tables with cos = 1, sin = 0; the float matrix keeps the sines
    "Pi": (0.5, -0.25, 0.125, 0.0, 0.0, 0.0),            # identity rotation, dyadic translation: the float transform of lattice points is exact
}

COMPONENTS = ["score"] + [f"g{i}" for i in range(6)] + [f"H{i}{j}" for i in range(6) for j in range(i, 6)]
TRI = [(i, j) for i in range(6) for j in range(i, 6)]


def gauss_constants_f32_options(resolution=1.0, outlier_ratio=0.55):
    """gauss_d1_, gauss_d2_ (ndt_omp_impl.hpp:86-93) from options held as floats, as smhip_ndt_options holds them."""
    return ondt.gauss_constants(float(F(resolution)), float(F(outlier_ratio)))[:2]


def pose_matrix_f32(p):
    """Translation(p0..2) * Rx * Ry * Rz in float (ndt_omp_impl.hpp:146-149, 803-806): float cosines and sines of the float angles,
    (Rx Ry) Rz with every product and sum rounded to float in turn, as Eigen's 3x3 products and the device's host code form them.
    oracle.ndt.pose_to_matrix_f32 is the same matrix through numpy's matmul, whose BLAS may fuse multiply-adds: it differs from
    this one in the last bit of an entry or two (at Pb: two entries), which moves every transformed point the same way -- a
    systematic 1e-8 of a gradient component that grows with the cloud, where N_c only covers independent ulps."""
    p = np.asarray(p, dtype=np.float64)
    a, b, c = F(p[3]), F(p[4]), F(p[5])
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    o, z = F(1), F(0)
    Rx = [[o, z, z], [z, ca, -sa], [z, sa, ca]]
    Ry = [[cb, z, sb], [z, o, z], [-sb, z, cb]]
    Rz = [[cc, -sc, z], [sc, cc, z], [z, z, o]]

    def mul(A, B):
        M = np.zeros((3, 3), dtype=F)
        for i in range(3):
            for j in range(3):
                s = F(0)
                for k in range(3):
                    s = F(s + F(A[i][k] * B[k][j]))
                M[i, j] = s
        return M
    T = np.eye(4, dtype=F)
    T[:3, :3] = mul(mul(Rx, Ry), Rz)
    T[:3, 3] = p[:3].astype(F)
    return T


def full_hessian(tri21, swap=True):
    """6x6 from the 21 upper-triangle components (row-major).  swap=False is ONE wrong mirror, not every one: below the diagonal
    the row-major index formula start(a) + (b - a) is applied to (a, b) as they stand, so the read lands before row a's first
    stored entry, in the tail of the rows above it -- H(1, 0) reads H(0, 5), H(5, 0) reads H(3, 3).  Those indices are 5 .. 19:
    the `% 21` never acts, it only says that the stand-in may not leave the array."""
    tri21 = np.asarray(tri21)
    H = np.zeros((6, 6), dtype=tri21.dtype)
    for a in range(6):
        for b in range(6):
            i, j = (min(a, b), max(a, b)) if swap else (a, b)
            H[a, b] = tri21[(i * 6 - i * (i - 1) // 2 + (j - i)) % 21]
    return H


def full_vector(v28, swap=True):
    """score, gradient and the mirrored Hessian as the 43 numbers a device returns."""
    v28 = np.asarray(v28)
    return np.concatenate([v28[:7], full_hessian(v28[7:], swap).reshape(-1)])


# ---------------------------------------------------------------------------------------------
# the voxel table from exact sums
# ---------------------------------------------------------------------------------------------
@dataclass
class Table:
    min_b: np.ndarray
    div_b: np.ndarray
    idx: np.ndarray          # [V, 3] voxel index from min_b, every occupied voxel, in key order (= the device's slot order)
    key: np.ndarray          # [V] i0 + i1 div0 + i2 div0 div1
    n: np.ndarray            # [V] points
    centroid: np.ndarray     # [V, 3] float32
    mean: np.ndarray         # [V, 3] float64
    icov: np.ndarray         # [V, 3, 3] float64 (zero where not searchable or not valid)
    valid: np.ndarray        # [V] eigenvalue check passed (searchable voxels)
    words: int               # 32-bit words of the dense occupancy grid
    eig: np.ndarray = None   # [V, 3] the covariance's eigenvalues, ascending, before the inflation of :346-356 (searchable voxels)

    def searchable(self, strict=False):
        return self.n > MIN_POINTS if strict else self.n >= MIN_POINTS


def finite_rows(cloud):
    return np.isfinite(np.asarray(cloud)[:, :3]).all(axis=1)


def check_lattice(cloud, quantum_of=None):
    """Every finite coordinate a multiple of its quantum, and n max|x| / quantum < 2^24 in every voxel."""
    p = np.asarray(cloud, dtype=np.float64)[:, :3]
    p = p[finite_rows(p)]
    vox = np.floor(p).astype(np.int64)
    _, inv, cnt = np.unique(vox, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    q = np.where(cnt[inv] > 64, Q8, Q10)
    assert (p / q[:, None] == np.round(p / q[:, None])).all()
    amax = np.zeros(len(cnt))
    np.maximum.at(amax, inv, np.abs(p).max(axis=1))
    qv = np.where(cnt > 64, Q8, Q10)
    assert (cnt * amax / qv < 2.0 ** 24).all()
    return True


def build_table(cloud) -> Table:
    pts32 = np.asarray(cloud, dtype=F)[:, :3]
    pts32 = pts32[finite_rows(pts32)]
    p = pts32.astype(np.float64)
    vox = np.floor(p).astype(np.int64)                       # resolution 1: p * inverse_leaf_size is p
    min_b, max_b = vox.min(axis=0), vox.max(axis=0)
    div_b = max_b - min_b + 1
    rel = vox - min_b
    key = rel[:, 0] + rel[:, 1] * div_b[0] + rel[:, 2] * div_b[0] * div_b[1]
    order = np.argsort(key, kind="stable")
    uk, start, cnt = np.unique(key[order], return_index=True, return_counts=True)
    V = len(uk)
    idx = rel[order][start]
    cent = np.zeros((V, 3), dtype=F); mean = np.zeros((V, 3)); icov = np.zeros((V, 3, 3)); valid = np.zeros(V, dtype=bool)
    eig = np.zeros((V, 3))
    ps = p[order]
    for v in range(V):
        q = ps[start[v]:start[v] + cnt[v]]
        n = int(cnt[v])
        s = q.sum(axis=0)                                    # exact (check_lattice)
        cent[v] = s.astype(F) / F(n)                         # the float sum is the same exact number, :241, :289
        mean[v] = s / n                                      # :293
        if n < MIN_POINTS:                                   # :297
            continue
        acc = np.eye(3) + q.T @ q                            # Leaf ctor cov_ = I, :235 (exact)
        cov = (acc - 2.0 * np.outer(s, mean[v])) / n + np.outer(mean[v], mean[v])      # :329
        cov *= (n - 1.0) / n                                 # :330
        w, E = np.linalg.eigh(cov)
        eig[v] = w
        if w[0] < 0 or w[1] < 0 or w[2] <= 0:                # :337-341
            continue
        m = EIG_MULT * w[2]
        if w[0] < m:                                         # :346-356
            w = w.copy(); w[0] = m
            if w[1] < m:
                w[1] = m
            cov = E @ np.diag(w) @ np.linalg.inv(E)
        ic = np.linalg.inv(cov)
        if np.isfinite(ic).all():
            icov[v] = ic; valid[v] = True
    words = int((div_b[0] + 31) // 32 * div_b[1] * div_b[2])
    return Table(min_b, div_b, idx, uk, cnt.astype(np.int64), cent, mean, icov, valid, words, eig)


# ---------------------------------------------------------------------------------------------
# targets
# ---------------------------------------------------------------------------------------------
def _voxel_points(rng, vox, n, quantum=Q10, lo=None, hi=None):
    """n lattice points strictly inside voxel `vox` (never on one of its planes)."""
    steps = int(round(1.0 / quantum))
    lo = np.array([1, 1, 1]) if lo is None else np.asarray(lo)
    hi = np.array([steps, steps, steps]) if hi is None else np.asarray(hi)
    f = rng.integers(lo, hi, size=(n, 3))
    return np.asarray(vox, dtype=np.float64) + f * quantum


@functools.lru_cache(maxsize=None)
def target(name):
    rng = np.random.default_rng({"block": 101, "strip": 102, "mixed": 103, "far": 104}[name])
    parts = []
    if name == "block":                                      # [-3, 3)^3, 8 points a voxel
        for z in range(-3, 3):
            for y in range(-3, 3):
                for x in range(-3, 3):
                    parts.append(_voxel_points(rng, (x, y, z), 8))
    elif name == "strip":                                    # 80 x 3 x 3 voxels: a row of the bit grid spans three words, min_b < 0
        for z in (-1, 0, 1):
            for y in (-1, 0, 1):
                for x in range(-40, 40):
                    parts.append(_voxel_points(rng, (x, y, z), 8))
    elif name == "mixed":
        for vox, n in MIXED_VOXELS.items():
            kind = MIXED_KIND.get(vox, "plain")
            if kind == "plain":
                parts.append(_voxel_points(rng, vox, n, Q8 if n > 64 else Q10))
            elif kind == "thin":                             # a slab 16 quanta thick: the smallest eigenvalue is inflated (:346-356)
                parts.append(_voxel_points(rng, vox, n, Q8, lo=(1, 1, 120), hi=(256, 256, 136)))
            elif kind == "coplanar":
                q = _voxel_points(rng, vox, n); q[:, 2] = vox[2] + 512 * Q10; parts.append(q)
            elif kind == "collinear":
                t = rng.permutation(np.arange(1, 1000, 7))[:n]
                parts.append(np.asarray(vox, dtype=np.float64) + np.stack([t, 1023 - t, t], axis=1) * Q10)
            elif kind == "identical":
                parts.append(np.repeat(_voxel_points(rng, vox, 1), n, axis=0))
        pts = np.concatenate(parts)
        pts = pts[rng.permutation(len(pts))]                 # a voxel's points are scattered over the cloud
        return np.concatenate([pts, np.zeros((len(pts), 1))], axis=1).astype(F)
    elif name == "far":                                      # two clusters 400 m apart on every axis: the dense box needs > 2^20 words
        parts = [_voxel_points(rng, (0, 0, 0), 8), _voxel_points(rng, (400, 400, 400), 8)]
    pts = np.concatenate(parts)
    return np.concatenate([pts, np.zeros((len(pts), 1))], axis=1).astype(F)


# voxel -> point count of the `mixed` target; every special voxel has no occupied neighbour but the ones listed next to it
MIXED_VOXELS = {
    (0, 0, 0): 5, (1, 0, 0): 8,                  # not searchable (a list entry all the same), with a searchable neighbour
    (3, 0, 0): 6, (-3, 0, 0): 7,                 # the min_points boundary
    (0, 3, 0): 2048, (0, -3, 0): 2049,           # both sides of the stats / stats_big split
    (3, 3, 0): 4000,                             # crowded and thin
    (-3, 3, 0): 12, (-3, -3, 0): 8, (3, -3, 0): 6,
    (0, 0, 3): 8, (1, 0, 3): 9, (0, 1, 3): 10, (0, 0, -3): 11, (-1, 0, -3): 8, (-1, -1, -3): 13,
}
MIXED_KIND = {(3, 3, 0): "thin", (-3, 3, 0): "coplanar", (-3, -3, 0): "collinear", (3, -3, 0): "identical"}


def with_nonfinite_rows(cloud):
    """`cloud` with three all-NaN rows and one row with a +Inf coordinate put in between."""
    c = np.asarray(cloud, dtype=F).copy()
    nan = np.full((1, c.shape[1]), np.nan, dtype=F)
    inf = c[7:8].copy(); inf[0, 1] = np.inf
    n = len(c)
    return np.concatenate([c[:n // 5], nan, c[n // 5:n // 2], inf, c[n // 2:n - 3], nan, nan, c[n - 3:]])


# ---------------------------------------------------------------------------------------------
# sources
# ---------------------------------------------------------------------------------------------
def transform_f32(src, T):
    """pcl::transformPointCloud with the float matrix, in the written order, without contraction."""
    x = np.asarray(src, dtype=F)[:, :3]
    T = np.asarray(T, dtype=F)
    with np.errstate(invalid="ignore"):
        return np.stack([((T[r, 0] * x[:, 0] + T[r, 1] * x[:, 1]) + T[r, 2] * x[:, 2]) + T[r, 3] for r in range(3)], axis=1).astype(F)


def find_pairs(table: Table, xt, strict=False):
    """(point, voxel) for every searchable voxel whose centroid lies within the resolution of the transformed point -- what
    radiusSearch returns (voxel_grid_covariance_omp.h:470-499) -- and the smallest | distance - resolution | met."""
    x = np.asarray(xt, dtype=np.float64)
    ok = np.isfinite(x).all(axis=1)
    sv = np.nonzero(table.searchable(strict))[0]
    d = np.sqrt(((np.where(ok[:, None], x, 0.0)[:, None, :] - table.centroid[sv].astype(np.float64)[None]) ** 2).sum(axis=2))
    d[~ok] = np.inf
    pi, k = np.nonzero(d <= RESOLUTION)
    gap = np.abs(d - RESOLUTION).min() if d.size else np.inf
    return pi, sv[k], gap


def list_entries(table: Table, xt):
    """Per query the occupied voxels (searchable or not) among the 27 around its voxel: the entries a wave lists."""
    x = np.asarray(xt, dtype=np.float64)
    ok = np.isfinite(x).all(axis=1)
    c = np.floor(np.where(ok[:, None], x, 0.0)).astype(np.int64) - table.min_b
    occ = set(map(tuple, table.idx.tolist()))
    out = np.zeros(len(x), dtype=np.int64)
    for i in np.nonzero(ok)[0]:
        if (c[i] < -1).any() or (c[i] > table.div_b).any():
            continue
        out[i] = sum((c[i, 0] + dx, c[i, 1] + dy, c[i, 2] + dz) in occ for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return out


def plane_gap(xt, exempt=None):
    x = np.asarray(xt, dtype=np.float64)
    ok = np.isfinite(x).all(axis=1)
    if exempt is not None:
        ok = ok & ~exempt
    x = x[ok]
    return np.abs(x - np.round(x)).min() if x.size else np.inf


def source_for(positions, pose):
    """Source rows whose float transform by `pose` lands (to rounding) on `positions`."""
    T = pose_matrix_f32(np.asarray(pose)).astype(np.float64)
    y = np.asarray(positions, dtype=np.float64)
    return ((y - T[:3, 3]) @ T[:3, :3]).astype(F)           # R^-1 = R^T to float rounding; the margins are checked on the real transform


@dataclass
class Case:
    name: str
    target: str
    pose_name: str
    src: np.ndarray                 # [ns, 4] float32, as uploaded (may hold non-finite rows)
    entries: int | None = None      # asserted total of list entries (single-wave cases)
    on_plane: np.ndarray | None = None
    notes: dict = field(default_factory=dict)

    @property
    def pose(self):
        return np.array(POSES[self.pose_name])


def _margins_hold(table, src, pose, on_plane=None):
    xt = transform_f32(src, pose_matrix_f32(np.asarray(pose)))
    if not plane_gap(xt, on_plane) > MARGIN:
        return False
    return find_pairs(table, xt)[2] > MARGIN


def _search(make, table, pose, seed0, on_plane=None):
    for s in range(seed0, seed0 + 400):
        src = make(np.random.default_rng(s))
        if _margins_hold(table, src, pose, on_plane):
            return src
    raise AssertionError("no seed satisfies the margins")


def _pad4(src3):
    return np.concatenate([np.asarray(src3, dtype=F), np.zeros((len(src3), 1), dtype=F)], axis=1)


# block: query voxels by how many of the 27 around them are occupied.  Per axis: 'i' interior (index 1..4 from min_b), 'f' the
# outermost voxel inside (0 or 5), 'o' one voxel outside (-1 or 6)
_KINDS = {27: "iii", 18: "iif", 12: "iff", 8: "fff", 9: "iio", 3: "ioo", 1: "ooo"}
# (64 points each) interior, face, edge, corner, outside-9, outside-3, outside-1
WINDOW_MIX = {
    "one_window": ({27: 12, 18: 16, 12: 16, 8: 12, 9: 4, 3: 2, 1: 2}, 944),
    "exactly_1024": ({27: 24, 18: 12, 12: 8, 8: 4, 9: 0, 3: 8, 1: 8}, 1024),
    "one_over_1025": ({27: 24, 18: 12, 12: 8, 8: 5, 9: 0, 3: 5, 1: 10}, 1025),
    "interior_64": ({27: 64}, 1728),
    "interior_256": ({27: 256}, None),           # four waves: 1728 each whatever the device's point order puts where
}
SIZES = (1, 15, 16, 17, 63, 65, 255, 257, 1025)


def _block_positions(rng, mix):
    pos = []
    for cnt, n in mix.items():
        for _ in range(n):
            axes = list(_KINDS[cnt]); rng.shuffle(axes)
            idx = [int(rng.integers(1, 5)) if a == "i" else int(rng.choice([0, 5])) if a == "f" else int(rng.choice([-1, 6])) for a in axes]
            pos.append(np.array(idx) - 3 + rng.uniform(0.05, 0.95, 3))
    pos = np.array(pos)
    return pos[rng.permutation(len(pos))]


def _strip_positions(rng):
    """Queries of the strip target (in the target frame) and which of them lie on lattice planes."""
    pos = []
    for ix in (0, 31, 32, 33, 63, 64, 79):                   # x index from min_b = -40: both ends of every occupancy word
        for _ in range(3):
            pos.append([-40 + ix + rng.uniform(0.05, 0.95), rng.uniform(-0.95, 0.95), rng.uniform(-0.95, 0.95)])
    one_out = [(-41, None, None), (40, None, None), (None, -2, None), (None, 2, None), (None, None, -2), (None, None, 2)]
    two_out = [(-42, None, None), (41, None, None), (None, -3, None), (None, 3, None), (None, None, -3), (None, None, 3)]
    for vox in one_out + two_out:                            # (one voxel outside: close to the box's face, so a centroid inside is in reach)
        for _ in range(2):
            base = [int(rng.integers(-39, 39)), 0, 0]
            p = [base[a] + rng.uniform(0.3, 0.7) if vox[a] is None else vox[a] + (rng.uniform(0.75, 0.95) if vox[a] < 0 else rng.uniform(0.05, 0.25))
                 for a in range(3)]
            pos.append(p)
    pos.append([1.0e4 + 0.37, 0.3, -0.2])                    # far outside: the row arithmetic must stay in range
    return np.array(pos)


_STRIP_PLANES = np.array([[-40.0, 0.5, 0.5], [0.0, 0.0, 0.0], [40.0, 0.25, -0.75], [-8.0, 2.0, 0.5], [24.0, -0.5, -1.0], [32.0, 1.0, 1.0],
                          [-9.0, -2.0, 2.0], [39.5, 1.5, -2.0]])


def _mixed_positions(rng):
    pos = []
    t = build_table(target("mixed"))
    for vox in MIXED_VOXELS:
        v = np.array(vox, dtype=np.float64)
        k = (t.idx + t.min_b == np.array(vox)).all(axis=1).argmax()
        pos.append(t.centroid[k].astype(np.float64) + rng.uniform(-0.3, 0.3, 3))     # in reach of the voxel's centroid
        for _ in range(3):                                   # and in voxels around it
            off = rng.integers(-1, 2, 3)
            pos.append(v + off + rng.uniform(0.1, 0.9, 3))
    return np.array(pos)


@functools.lru_cache(maxsize=None)
def tables():
    return {name: build_table(target(name)) for name in ("block", "strip", "mixed")}


def case_names():
    """The cases' names, without building them."""
    names = [f"block/{w}/{pn}" for pn in ("Pa", "Pb", "Pc") for w in WINDOW_MIX]
    names += [f"block/ns{ns}/{pn}" for ns in SIZES for pn in ("Pa", "Pb", "Pc")]
    names += [f"strip/{pn}" for pn in ("Pa", "Pb", "Pc", "Pi")] + [f"mixed/{pn}" for pn in ("Pa", "Pb", "Pc")]
    return names


def case(name):
    return {c.name: c for c in cases()}[name]


@functools.lru_cache(maxsize=None)
def cases():
    tb = tables()
    out = []
    seed = 1000
    for pn in ("Pa", "Pb", "Pc"):
        pose = POSES[pn]
        for name, (mix, total) in WINDOW_MIX.items():
            seed += 1000
            src = _search(lambda rng: source_for(_block_positions(rng, mix), pose), tb["block"], pose, seed)
            out.append(Case(f"block/{name}/{pn}", "block", pn, _pad4(src), entries=total))
    for ns in SIZES:
        seed += 1000
        # one source for the three poses: the margins must hold under each
        for s in range(seed, seed + 2000):
            src = np.random.default_rng(s).uniform(-3.9, 3.9, (ns, 3)).astype(F)
            if all(_margins_hold(tb["block"], src, POSES[pn]) for pn in ("Pa", "Pb", "Pc")):
                break
        else:
            raise AssertionError("no seed satisfies the margins")
        for pn in ("Pa", "Pb", "Pc"):
            out.append(Case(f"block/ns{ns}/{pn}", "block", pn, _pad4(src)))
    for pn in ("Pa", "Pb", "Pc", "Pi"):
        pose = POSES[pn]
        seed += 1000

        def make(rng, pose=pose, pn=pn):
            pos = _strip_positions(rng)
            if pn == "Pi":
                pos = np.concatenate([np.round(pos * 1024) / 1024, _STRIP_PLANES])   # lattice queries: an exact float transform
            return source_for(pos, pose)
        nplane = len(_STRIP_PLANES) if pn == "Pi" else 0
        nq = len(_strip_positions(np.random.default_rng(0))) + nplane
        on_plane = np.zeros(nq, dtype=bool)
        if nplane:
            on_plane[-nplane:] = True
        src = _pad4(_search(make, tb["strip"], pose, seed, on_plane))
        # two NaN rows and one Inf row in between: skipped, and the pair count says so
        bad = np.full((3, 4), np.nan, dtype=F); bad[1] = src[5]; bad[1, 0] = np.inf
        keep = np.concatenate([on_plane[:10], [False], on_plane[10:20], [False, False], on_plane[20:]])
        src = np.concatenate([src[:10], bad[:1], src[10:20], bad[1:], src[20:]])
        out.append(Case(f"strip/{pn}", "strip", pn, src, on_plane=keep))
    for pn in ("Pa", "Pb", "Pc"):
        pose = POSES[pn]
        seed += 1000
        src = _search(lambda rng: source_for(_mixed_positions(rng), pose), tb["mixed"], pose, seed)
        out.append(Case(f"mixed/{pn}", "mixed", pn, _pad4(src)))
    assert [c.name for c in out] == case_names()
    return tuple(out)


def case_xt(case: Case):
    return transform_f32(case.src, pose_matrix_f32(case.pose))


# ---------------------------------------------------------------------------------------------
# the reference evaluation
# ---------------------------------------------------------------------------------------------
def evaluate(table: Table, src, xt, pose, d1, d2, double_math, hessian=True, pairs=None, mutate=None):
    """One computeDerivatives in float64 from what a device is given: float32 source rows and transformed points, the table's
    double means, its icov rounded to float32 (float path) or as it is (double path), the angle tables in the path's type.
    Returns (values[28], A[28], pair count, (pi, vi), e[pairs]).  `mutate` names one deliberately wrong kernel (tests)."""
    real = np.float64 if double_math else None
    j_ang, h_ang = ondt.angle_derivatives(np.asarray(pose, dtype=np.float64), real)
    j_ang = j_ang.astype(np.float64)[:, :3]; h_ang = h_ang.astype(np.float64)[:15, :3].copy()
    if mutate == "h_ang_rows_9_12":
        h_ang[[9, 12]] = h_ang[[12, 9]]
    gd2 = float(d2) if double_math else float(F(d2))
    if pairs is None:
        pi, vi, _ = find_pairs(table, xt, strict=(mutate == "min_points_le"))
    else:
        pi, vi = pairs
    vals = np.zeros(28); A = np.zeros(28)
    if len(pi) == 0:
        return vals, A, 0, (pi, vi), np.zeros(0)
    icov = table.icov if double_math else table.icov.astype(F).astype(np.float64)
    C = icov[(vi + 1) % len(icov)] if mutate == "icov_next_slot" else icov[vi]
    x = np.asarray(src, dtype=F)[:, :3].astype(np.float64)[pi]
    u = np.asarray(xt, dtype=F).astype(np.float64)[pi] - table.mean[vi]            # :253, :490
    v = np.einsum("kij,kj->ki", C, u)                                              # x_trans' C
    q = (u * v).sum(axis=1)
    e0 = np.exp(-gd2 * q / 2)                                                      # :497
    e1 = gd2 * e0                                                                  # :501
    good = ~((e1 > 1) | (e1 < 0) | np.isnan(e1))                                   # :504-505
    inc = np.where(good, -d1 * e0, 0.0)                                            # :499
    e = np.where(good, d1 * e1, 0.0)                                               # :508
    if mutate == "drop_weakest_pair":
        keep = np.ones(len(pi), dtype=bool); keep[np.argmin(np.abs(e))] = False
        pi, vi, C, x, u, v, inc, e = pi[keep], vi[keep], C[keep], x[keep], u[keep], v[keep], inc[keep], e[keep]
    npairs = len(pi)
    pg = x @ j_ang.T                                                               # :403
    J = np.zeros((npairs, 3, 6))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1
    J[:, 1, 3] = pg[:, 0]; J[:, 2, 3] = pg[:, 1]
    J[:, 0, 4] = pg[:, 2]; J[:, 1, 4] = pg[:, 3]; J[:, 2, 4] = pg[:, 4]
    J[:, 0, 5] = pg[:, 5]; J[:, 1, 5] = pg[:, 6]; J[:, 2, 5] = pg[:, 7]
    xCJ = np.einsum("ki,kil->kl", v, J)                                            # :511
    vals[0] = inc.sum(); A[0] = np.abs(inc).sum()
    gt = e[:, None] * xCJ                                                          # :513
    vals[1:7] = gt.sum(axis=0); A[1:7] = np.abs(gt).sum(axis=0)
    if hessian:
        ph = x @ h_ang.T                                                           # :416
        z = np.zeros(npairs)
        a = np.stack([z, ph[:, 0], ph[:, 1]], axis=1); b = np.stack([z, ph[:, 2], ph[:, 3]], axis=1); c = np.stack([z, ph[:, 4], ph[:, 5]], axis=1)
        d = ph[:, 6:9]; ee = ph[:, 9:12]; f = ph[:, 12:15]
        PH = np.zeros((npairs, 6, 6, 3))
        PH[:, 3, 3] = a; PH[:, 4, 3] = b; PH[:, 5, 3] = c
        PH[:, 3, 4] = b; PH[:, 4, 4] = d; PH[:, 5, 4] = ee
        PH[:, 3, 5] = c; PH[:, 4, 5] = ee; PH[:, 5, 5] = f
        t1 = -(1.0 if mutate == "no_d2_in_W" else gd2) * xCJ[:, :, None] * xCJ[:, None, :]     # :527
        t2 = np.einsum("kc,kijc->kij", v, PH)                                                  # :523, :528
        t3 = np.einsum("kci,kcd,kdj->kij", J, C, J)                                            # :517, :529
        Hs = (e[:, None, None] * (t1 + t2 + t3)).sum(axis=0)
        Ha = (np.abs(e[:, None, None] * t1) + np.abs(e[:, None, None] * t2) + np.abs(e[:, None, None] * t3)).sum(axis=0)
        vals[7:] = [Hs[i, j] for i, j in TRI]; A[7:] = [Ha[i, j] for i, j in TRI]
    return vals, A, npairs, (pi, vi), e


@dataclass
class Reference:
    values: np.ndarray       # [28]
    A: np.ndarray            # [28]
    N: np.ndarray            # [28]
    S: np.ndarray            # [28] u A + N
    pairs: int
    pair_index: tuple
    e: np.ndarray

    def full(self, swap=True):
        return full_vector(self.values, swap)

    def full_scale(self):
        return full_vector(self.S)


def _ulp_moves(xt, seed):
    rng = np.random.default_rng(seed)
    x = np.asarray(xt, dtype=F)
    step = rng.integers(-1, 2, size=x.shape)
    with np.errstate(invalid="ignore"):
        up, dn = np.nextafter(x, F(np.inf)), np.nextafter(x, F(-np.inf))
    return np.where(step > 0, up, np.where(step < 0, dn, x)).astype(F)


def reference(table: Table, src, xt, pose, d1, d2, double_math, hessian=True) -> Reference:
    vals, A, npairs, pairs, e = evaluate(table, src, xt, pose, d1, d2, double_math, hessian)
    N = np.zeros(28)
    for t in range(16):
        moved, _, _, _, _ = evaluate(table, src, _ulp_moves(xt, 7000 + t), pose, d1, d2, double_math, hessian, pairs=pairs)
        N = np.maximum(N, np.abs(moved - vals))
    u = 2.0 ** -53 if double_math else 2.0 ** -24
    return Reference(vals, A, N, u * A + N, npairs, pairs, e)


def case_reference(case: Case, d1, d2, double_math, hessian=True) -> Reference:
    return reference(tables()[case.target], case.src, case_xt(case), case.pose, d1, d2, double_math, hessian)


def worst_ratio(got43, ref: Reference, swap=True):
    """max over the 43 returned numbers of |got - ref| / S (0 / 0 counts as 0), and where."""
    diff = np.abs(np.asarray(got43, dtype=np.float64) - ref.full(swap))
    S = ref.full_scale()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / S)
    k = int(np.argmax(r))
    return float(r[k]), k


MUTATIONS = ("h_ang_rows_9_12", "no_d2_in_W", "mirror_not_swapped", "icov_next_slot", "drop_weakest_pair", "min_points_le")
