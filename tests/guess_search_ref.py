"""The correlative guess search of DESIGN.md §6 ("Guess search") restated in numpy, rule by rule (include/smhip.h states the same
rules).  Everything after rule 5 is integer, so the device has to give these scores cell for cell.

Float conventions that matter: rule 3 / 5 divide in float32 (IEEE, numpy's float32 division) and floor; rule 5 rounds every float32
product and sum on its own, in the order ((r0 x + r1 y) + r2 z) + t; rule 4 forms Rz(a step) R0 in Python floats (doubles) with
math.cos / math.sin -- the C library's, as the host code's are -- every product and sum rounded, and casts to float32."""
import math

import numpy as np

MAX_CANDIDATES = 1 << 25
MAX_BITMAP_BITS = 1 << 28
MAX_HALF = 1 << 19
FIELD = 1 << 20
MAX_VOXEL = 1 << 30
DEFAULTS = dict(resolution=0.5, max_source_points=4096, half_xy=20, half_z=2, yaw_steps=10, yaw_step=2.0 * math.pi / 180.0)


class Refused(Exception):
    def __init__(self, status, why):
        super().__init__(why)
        self.status = status            # "invalid" (SMHIP_ERR_INVALID_ARGUMENT) or "capacity" (SMHIP_ERR_CAPACITY)


def finite_rows(cloud):
    """rule 1: the x y z of the rows whose x, y and z are finite, as float32, in order"""
    c = np.asarray(cloud, np.float32)
    return np.ascontiguousarray(c[np.isfinite(c[:, :3]).all(axis=1)][:, :3])


def sample_rows(n, M):
    """rule 2: the indices kept of n rows"""
    if n <= M:
        return np.arange(n, dtype=np.int64)
    return (np.arange(M, dtype=np.int64) * np.int64(n)) // np.int64(M)


def voxels(p, res):
    """rule 3: floor(p / res) per axis in float32, as int64; Refused("capacity") when one does not fit"""
    with np.errstate(all="ignore"):
        f = np.floor(np.asarray(p, np.float32) / np.float32(res))
    if not (np.abs(f) < np.float32(MAX_VOXEL)).all():          # (false for a NaN too)
        raise Refused("capacity", "a voxel coordinate does not fit the index type")
    return f.astype(np.int64)


def yaw_transform(guess, angle):
    """rule 4: (R [3, 3], t [3]) of Rz(angle) R0, t0 in doubles"""
    g = np.asarray(guess, np.float64).reshape(4, 4)
    c, s = math.cos(angle), math.sin(angle)
    R = np.zeros((3, 3))
    for col in range(3):
        r0, r1, r2 = float(g[0, col]), float(g[1, col]), float(g[2, col])
        R[0, col] = c * r0 - s * r1
        R[1, col] = s * r0 + c * r1
        R[2, col] = r2
    return R, g[:3, 3].copy()


def transform_f32(R, t, p):
    """rule 5: q = ((r0 x + r1 y) + r2 z) + t in float32, every operation rounded on its own"""
    R32, t32 = R.astype(np.float32), t.astype(np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((R32[r, 0] * x + R32[r, 1] * y) + R32[r, 2] * z) + t32[r] for r in range(3)], axis=1)


def check(n_target, n_source, o, guess, max_points=None):
    if n_target < 1 or n_source < 1:
        raise Refused("invalid", "a cloud with no row")
    res = float(np.float32(o["resolution"]))
    if not math.isfinite(res) or not res > 0:
        raise Refused("invalid", "resolution")
    if o["half_xy"] < 0 or o["half_z"] < 0 or o["yaw_steps"] < 0:
        raise Refused("invalid", "a negative window")
    if not math.isfinite(o["yaw_step"]):
        raise Refused("invalid", "yaw_step")
    if o["max_source_points"] < 1:
        raise Refused("invalid", "max_source_points")
    if not np.isfinite(np.asarray(guess, np.float64)).all():
        raise Refused("invalid", "the guess is not finite")
    if max(o["half_xy"], o["half_z"], o["yaw_steps"]) > MAX_HALF:
        raise Refused("capacity", "a half-width above 2^19")
    nxy, nz, nyaw = 2 * o["half_xy"] + 1, 2 * o["half_z"] + 1, 2 * o["yaw_steps"] + 1
    if nxy * nxy * nz * nyaw > MAX_CANDIDATES:
        raise Refused("capacity", "more than 2^25 candidates")
    if max_points is not None and max(n_target, n_source) > max_points:
        raise Refused("capacity", "a cloud larger than the handle's capacity")
    return nxy, nz, nyaw


def pick(volume, half_xy, half_z, yaw_steps):
    """rules 7 and 9 on a volume [nyaw, nz, nxy, nxy]: ((a, i, j, k), best_score, runner_up_score)"""
    a, k, j, i = np.meshgrid(np.arange(-yaw_steps, yaw_steps + 1), np.arange(-half_z, half_z + 1), np.arange(-half_xy, half_xy + 1),
                             np.arange(-half_xy, half_xy + 1), indexing="ij")
    best = int(volume.max())
    at = volume == best
    keys = np.stack([(i * i + j * j + k * k)[at], np.abs(a)[at], a[at], k[at], j[at], i[at]], axis=1).astype(np.int64)
    first = keys[np.lexsort(keys.T[::-1])[0]]
    a_, k_, j_, i_ = (int(v) for v in first[2:])
    apart = (np.maximum(np.maximum(np.abs(i - i_), np.abs(j - j_)), np.abs(k - k_)) > 2) | (np.abs(a - a_) > 1)
    runner_up = int(volume[apart].max()) if apart.any() else 0
    return (a_, i_, j_, k_), best, runner_up


def search(target, source, guess, max_points=None, **options):
    """The whole definition.  Returns a dict: transform [4, 4] float64, best (a, i, j, k), best_score, guess_score, runner_up_score,
    n_source_used, n_candidates, volume int32 [nyaw, nz, nxy, nxy], origin / extent (the bitmap's box), voxels int64 [nyaw, m, 3] (w of
    rule 5) and reachable bool [nyaw, m] (can an offset of the window bring the point into the box)."""
    o = dict(DEFAULTS)
    o.update(options)
    target, source = np.asarray(target, np.float32), np.asarray(source, np.float32)
    for c in (target, source):
        if c.ndim != 2 or c.shape[1] not in (4, 5):
            raise Refused("invalid", "a bad stride")
    nxy, nz, nyaw = check(len(target), len(source), o, guess, max_points)
    hxy, hz, Ky = o["half_xy"], o["half_z"], o["yaw_steps"]
    res = np.float32(o["resolution"])
    tgt, src = finite_rows(target), finite_rows(source)
    if len(tgt) == 0 or len(src) == 0:
        raise Refused("invalid", "a cloud has no finite row")
    src = src[sample_rows(len(src), o["max_source_points"])]
    m = len(src)
    v = voxels(tgt, res)
    origin, extent = v.min(axis=0), v.max(axis=0) - v.min(axis=0) + 1
    for c, half in zip(range(3), (hxy, hxy, hz)):
        if extent[c] + half > FIELD:
            raise Refused("capacity", "the box and the window do not fit a packed voxel field")
    if ((int(extent[0]) + 31) // 32) * 32 * int(extent[1]) * int(extent[2]) > MAX_BITMAP_BITS:
        raise Refused("capacity", "a bitmap above 2^28 bits")
    ex, ey, ez = (int(e) for e in extent)
    # occupancy padded by two half-widths on every side: a reachable point's whole window is then a plain slice
    occ = np.zeros((ez + 4 * hz, ey + 4 * hxy, ex + 4 * hxy), np.int32)
    r = v - origin
    occ[r[:, 2] + 2 * hz, r[:, 1] + 2 * hxy, r[:, 0] + 2 * hxy] = 1
    volume = np.zeros((nyaw, nz, nxy, nxy), np.int32)
    all_w = np.zeros((nyaw, m, 3), np.int64)
    reach = np.zeros((nyaw, m), bool)
    for a in range(-Ky, Ky + 1):
        R, t = yaw_transform(guess, a * o["yaw_step"])
        w = voxels(transform_f32(R, t, src), res)
        all_w[a + Ky] = w
        q = w - origin
        ok = ((q[:, 0] >= -hxy) & (q[:, 0] < ex + hxy) & (q[:, 1] >= -hxy) & (q[:, 1] < ey + hxy) & (q[:, 2] >= -hz) & (q[:, 2] < ez + hz))
        reach[a + Ky] = ok
        cells, counts = np.unique(q[ok], axis=0, return_counts=True)
        vol = volume[a + Ky]
        for (x, y, z), n in zip(cells, counts):
            # offset (i, j, k) looks at relative voxel (x + i, y + j, z + k): padded index x + i + 2 hxy, i = -hxy .. hxy
            vol += n * occ[z + hz:z + hz + nz, y + hxy:y + hxy + nxy, x + hxy:x + hxy + nxy]
    (a_, i_, j_, k_), best, runner_up = pick(volume, hxy, hz, Ky)
    R, t = yaw_transform(guess, a_ * o["yaw_step"])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t + float(res) * np.array([i_, j_, k_], np.float64)
    return dict(transform=T, best=(a_, i_, j_, k_), best_score=best, guess_score=int(volume[Ky, hz, hxy, hxy]), runner_up_score=runner_up,
                n_source_used=m, n_candidates=nyaw * nz * nxy * nxy, volume=volume, origin=origin, extent=extent, voxels=all_w, reachable=reach)


def score_brute(target, source, guess, a, i, j, k, **options):
    """rule 6 for one candidate, straight from the words of the definition (a set of occupied voxels): checks search() itself"""
    o = dict(DEFAULTS)
    o.update(options)
    res = np.float32(o["resolution"])
    tgt, src = finite_rows(target), finite_rows(source)
    src = src[sample_rows(len(src), o["max_source_points"])]
    occupied = set(map(tuple, voxels(tgt, res).tolist()))
    R, t = yaw_transform(guess, a * o["yaw_step"])
    w = voxels(transform_f32(R, t, src), res)
    return sum((int(x) + i, int(y) + j, int(z) + k) in occupied for x, y, z in w)
