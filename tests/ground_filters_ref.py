"""CPU restatement of the reference's GroundRemoval, GroundRemoval2 and RangeImage filters (numpy / Python), the yardstick of
the device kernels in staticmapping_amd/csrc/ground_filters.hip.

Restates (paths relative to the reference's pre_processors/)
  filter_ground_removal.cc:51-112     GroundRemoval::SetInputCloud / Filter
  filter_ground_removal2.cc:28-70     FitLocalLine, GetMaxError, LocalLineToLine
  filter_ground_removal2.cc:134-192   GroundRemoval2::SetInputCloud (binning, grid membership)
  filter_ground_removal2.cc:236-309   GroundRemoval2::FitLines
  filter_ground_removal2.cc:316-397   GroundRemoval2::ClusterGround, VerticalDistanceToSegment
  filter_range_image.cc:75-126        RangeImage::Filter
Clouds are float32 [N, 5] InnerPointType rows (x, y, z, intensity, factor); each filter returns a keep mask in input order.

What is pinned and what is not ("Pre-filters"):
  * FitLocalLine: the reference solves with Eigen's colPivHouseholderQr in double.  Here (and on the device) the centred normal
    equations in double with one fixed summation order (`fit_line`); checked against numpy.linalg.lstsq, not against Eigen.
  * Angles: (float)atan2((double)y, (double)x) instead of glibc's atan2f, which may differ by an ulp at a bin / pixel boundary.
  * float -> int: x86's truncation, INT_MIN for NaN and out-of-range values (`trunc_x86`).
  * Non-finite rows (x, y or z): kept by both ground filters, dropped by RangeImage (the reference's result depends on NaN
    conversions and, for GroundRemoval2, can stop in a CHECK).
  * Output order: input order for all three (GroundRemoval emits voxel by voxel in the reference).
"""
from __future__ import annotations

import numpy as np

from oracle import filters as of

F = np.float32
INT_MIN = -2 ** 31
GROUND_REMOVAL, GROUND_REMOVAL2, RANGE_IMAGE = 6, 7, 8
VOX_BIAS = 1 << 20

GR_DEFAULTS = dict(leaf_size=0.8, height_threshold=0.15, min_point_num_in_voxel=10)            # filter_ground_removal.cc:28-31
GR2_DEFAULTS = dict(r_max=100.0, r_min=1.0, bin_num=200, segment_num=180, start_ground_height=-0.25,  # filter_ground_removal2.cc:72-88
                    long_line_threshold=1.0, max_long_line_height=0.1, max_start_height=0.2, max_error=0.05,
                    max_slope=float(F(np.tan(np.pi / 12.0))), max_b=0.1, max_dist_to_line=0.05, search_angle=10.0, thread_num=4)
RI_DEFAULTS = dict(top_angle=30.0, btm_angle=-15.0, offset_x=0.0, offset_y=0.0, offset_z=0.0,   # filter_range_image.cc:28-35
                   vertical_line_num=40, horizontal_line_num=1800)


def trunc_x86(v) -> np.ndarray:
    """static_cast<int> as x86 runs it: truncation; INT_MIN for NaN and for values outside the int range"""
    v = np.asarray(v)
    with np.errstate(invalid="ignore"):
        if v.dtype == np.float32:
            ok = (v >= -2147483648.0) & (v < 2147483648.0)
        else:
            ok = (v > -2147483649.0) & (v < 2147483648.0)
        return np.where(ok, np.trunc(np.where(ok, v, 0)), INT_MIN).astype(np.int64)


def angle_f(y, x) -> np.ndarray:
    """(float)atan2((double)y, (double)x): the device's angle (the reference: glibc atan2f)"""
    return np.arctan2(np.asarray(y, np.float64), np.asarray(x, np.float64)).astype(F)


def finite_rows(pts) -> np.ndarray:
    return np.isfinite(pts[:, 0]) & np.isfinite(pts[:, 1]) & np.isfinite(pts[:, 2])


# ---- GroundRemoval2 ------------------------------------------------------------------------------------------------------
def _wave_sum(v: np.ndarray) -> float:
    """the device's xor butterfly over 64 lanes: halves added pairwise, 32 + 32, 16 + 16, ..."""
    while len(v) > 1:
        h = len(v) // 2
        v = v[:h] + v[h:]
    return float(v[0])


def _lane_sums(v: np.ndarray) -> float:
    """lane j adds elements j, j + 64, ... in turn (from 0.0), then the butterfly"""
    rows = -(-len(v) // 64)
    pad = np.zeros(rows * 64)
    pad[:len(v)] = v
    acc = np.zeros(64)
    for r in range(rows):
        acc = acc + pad[64 * r:64 * (r + 1)]
    return _wave_sum(acc)


def fit_line_f64(d, z):
    """FitLocalLine, filter_ground_removal2.cc:28-43, restated: the least-squares line z = m d + b through the points by the
    centred normal equations in double, m = Sdz / Sdd, b = mean_z - m mean_d, summed in the device's order.
    (The reference: Eigen colPivHouseholderQr; the two agree to rounding, not bit for bit.)"""
    d = np.asarray(d, np.float64)
    z = np.asarray(z, np.float64)
    L = len(d)
    md = _lane_sums(d) / L
    mz = _lane_sums(z) / L
    dd, dz = d - md, z - mz
    m = _lane_sums(dd * dz) / _lane_sums(dd * dd)
    return m, mz - m * md


def fit_line(d, z):
    """fit_line_f64 with m and b stored as float, as LocalLine holds them"""
    m, b = fit_line_f64(d, z)
    return F(m), F(b)


def max_error(d32, z32, m, b) -> F:
    """GetMaxError, :45-55 (float)"""
    e = np.abs(m * d32 + b - z32)
    return F(max(F(0), e.max()))


def gr2_params(**kw) -> dict:
    p = dict(GR2_DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def gr2_search_step(search_angle, segment_num) -> int:
    """ClusterGround, :318-320: delta_alpha = (float)(M_PI * 2 / segment_num_); search_angle_ / 180. * M_PI / delta_alpha"""
    da = float(F(np.pi * 2 / segment_num))
    return int(trunc_x86(np.float64(float(F(search_angle)) / 180.0 * np.pi / da)))


def gr2_bin(pts: np.ndarray, p: dict):
    """SetInputCloud, :146-177: grid index per row (-1 = non-finite row), range d and z (float32)"""
    B, S = int(p["bin_num"]), int(p["segment_num"])
    x, y, z = (np.asarray(pts[:, k], F) for k in range(3))
    fin = finite_rows(pts)
    two_pi = F(np.pi * 2)                                       # const float double_pi = M_PI * 2
    da = two_pi / F(S)
    db = (F(p["r_max"]) - F(p["r_min"])) / F(B)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rng = np.sqrt(x * x + y * y)
        rad = angle_f(y, x)
        rad = np.where(rad < 0, rad + two_pi, rad).astype(F)
        s = np.clip(trunc_x86((rad / da).astype(F)), 0, S - 1)  # :171-180: clamp (INT_MIN -> 0)
        b = np.clip(trunc_x86(((rng - F(p["r_min"])) / db).astype(F)), 0, B - 1)
    grid = np.where(fin, s * B + b, -1)
    return grid, rng, z


def gr2_grids(grid, rng, z):
    """:181-191 in input order: update the minimum (empty grid or z < min), then join if z <= min + 0.5 (double).
    Returns member mask and {grid: (d, z) of min_z_point}."""
    member = np.zeros(len(grid), bool)
    gmin = {}
    gl, dl, zl = grid.tolist(), rng.tolist(), z.tolist()       # python floats hold the float32 values exactly
    for i in range(len(gl)):
        g = gl[i]
        if g < 0:
            continue
        cur = gmin.get(g)
        if cur is None or zl[i] < cur[1]:
            cur = (dl[i], zl[i])
            gmin[g] = cur
        if zl[i] <= cur[1] + 0.5:
            member[i] = True
    return member, gmin


def gr2_fit_lines(gmin: dict, seg: int, p: dict) -> np.ndarray:
    """FitLines, :236-309, for one segment: lines (start d, start z, end d, end z) float32 [L, 4]"""
    B = int(p["bin_num"])
    long_thr, long_h = F(p["long_line_threshold"]), F(p["max_long_line_height"])
    max_err, max_slope, start_max = F(p["max_error"]), F(p["max_slope"]), F(p["max_start_height"])
    bins = [(F(v[0]), F(v[1])) for v in (gmin.get(seg * B + b) for b in range(B)) if v is not None]
    first = next((b for b in range(B) if seg * B + b in gmin), B)
    lines = []
    if first >= B - 1:                                          # :246-248
        return np.zeros((0, 4), F)
    P = [bins[0]]
    cm, cb = F(0), F(0)
    is_long = False
    gh = F(p["start_ground_height"])

    def emit(pts_):
        nm, nb = fit_line([q[0] for q in pts_], [q[1] for q in pts_])
        sd, ed = pts_[0][0], pts_[-1][0]
        lines.append((sd, F(nm * sd + nb), ed, F(nm * ed + nb)))
        return nm, nb

    k = 1
    while k < len(bins):
        cp = bins[k]
        if cp[0] - P[-1][0] >= long_thr:                        # :265-268
            is_long = True
        ez = F(np.finfo(F).max)
        if is_long and len(P) > 2:
            ez = F(cm * cp[0] + cb)
        if len(P) >= 2:
            P.append(cp)
            cm, cb = fit_line([q[0] for q in P], [q[1] for q in P])
            d32 = np.array([q[0] for q in P], F)
            z32 = np.array([q[1] for q in P], F)
            err = max_error(d32, z32, cm, cb)
            if err > max_err or abs(cm) > max_slope or (is_long and abs(F(ez - cp[1])) > long_h):
                P.pop()
                if len(P) >= 3:
                    nm, nb = emit(P)
                    gh = F(nm * P[-1][0] + nb)                  # :288-289
                is_long = False
                P = [P[-1]]
                continue                                        # --i: the same bin again
        else:
            if not is_long and abs(F(P[-1][1] - gh)) < start_max:
                P.append(cp)
            else:
                P = [cp]
        k += 1
    if len(P) > 2:
        emit(P)
    return np.array(lines, F).reshape(-1, 4)


def vertical_distance(d, z, lines) -> np.ndarray:
    """VerticalDistanceToSegment, :379-397: the last covering line wins; -1 where none covers"""
    margin = F(0.1)
    dist = np.full(len(d), F(-1), F)
    for l in lines:
        cover = (l[0] - margin < d) & (l[2] + margin > d)
        dz, dd = F(l[3] - l[1]), F(l[2] - l[0])
        ez = ((d - l[0]) / dd * dz + l[1]).astype(F)
        dist = np.where(cover, np.abs(z - ez), dist).astype(F)
    return dist


def ground_removal2(pts: np.ndarray, **kw) -> np.ndarray:
    """GroundRemoval2::Filter: keep mask in input order (non-finite rows kept)"""
    p = gr2_params(**kw)
    B, S = int(p["bin_num"]), int(p["segment_num"])
    pts = np.asarray(pts, F)
    grid, rng, z = gr2_bin(pts, p)
    member, gmin = gr2_grids(grid, rng, z)
    lines = [gr2_fit_lines(gmin, s, p) for s in range(S)]
    step = gr2_search_step(p["search_angle"], S)
    remove = np.zeros(len(pts), bool)
    seg_of = np.where(grid >= 0, grid // B, -1)
    for s in range(S):
        ids = np.flatnonzero(member & (seg_of == s))
        if len(ids) == 0:
            continue
        d, zz = rng[ids], z[ids]
        dist = vertical_distance(d, zz, lines[s])
        todo = dist < 0
        for k in range(step, 0, -1):                             # candidates +k, -k, ..., +1, -1; stop at the first distance > 0
            for c in (s + k, s - k):
                if not todo.any():
                    break
                c = c + S if c < 0 else (c - S if c >= S else c)
                sel = np.flatnonzero(todo)
                dist[sel] = vertical_distance(d[sel], zz[sel], lines[c])
                todo[sel[dist[sel] > 0]] = False
        remove[ids] = (dist > 0) & (dist <= F(p["max_dist_to_line"]))
    return ~remove


# ---- GroundRemoval -------------------------------------------------------------------------------------------------------
def ground_removal(pts: np.ndarray, leaf_size=0.8, height_threshold=0.15, min_point_num_in_voxel=10) -> np.ndarray:
    """GroundRemoval: keep mask in input order (non-finite rows kept).  Voxel = static_cast<int>(coord / leaf) per axis."""
    pts = np.asarray(pts, F)
    leaf = F(leaf_size)
    fin = finite_rows(pts)
    keep = np.ones(len(pts), bool)
    ids = np.flatnonzero(fin)
    if len(ids) == 0:
        return keep
    with np.errstate(over="ignore"):
        ijk = np.stack([trunc_x86((pts[ids, k] / leaf).astype(F)) for k in range(3)], axis=1)
    if np.any((ijk < -VOX_BIAS) | (ijk >= VOX_BIAS)):
        raise ValueError("voxel index beyond +-2^20 (refused by the device)")
    vox, inv, cnt = np.unique(ijk, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    z = pts[ids, 2]
    zmax = np.full(len(vox), -np.inf, F)
    zmin = np.full(len(vox), np.inf, F)
    np.maximum.at(zmax, inv, z)
    np.minimum.at(zmin, inv, z)
    mx = np.where(zmax > F(-1.e9), zmax, F(-1.e9)).astype(F)   # the reference starts at -1e9 / 1e9, :82-83
    mn = np.where(zmin < F(1.e9), zmin, F(1.e9)).astype(F)
    delta = (mx - mn).astype(F)
    ground = (vox[:, 2] <= 0) & (delta >= 0) & (delta <= F(height_threshold))
    keep_vox = (cnt >= int(min_point_num_in_voxel)) & ~ground
    keep[ids] = keep_vox[inv]
    return keep


# ---- RangeImage ----------------------------------------------------------------------------------------------------------
def range_image_pixels(pts: np.ndarray, top_angle=30.0, btm_angle=-15.0, offset_x=0.0, offset_y=0.0, offset_z=0.0,
                       vertical_line_num=40, horizontal_line_num=1800) -> np.ndarray:
    """RangeImage::Filter, :84-115: the pixel (row * H + col) of every row, -1 when the row is dropped"""
    V, H = int(vertical_line_num), int(horizontal_line_num)
    pts = np.asarray(pts, F)
    fin = finite_rows(pts)
    with np.errstate(invalid="ignore", over="ignore"):
        x = pts[:, 0] + F(offset_x)
        y = pts[:, 1] + F(offset_y)
        z = pts[:, 2] + F(offset_z)
        dxy = np.sqrt(x * x + y * y)
        hres = F(np.pi * 2 / float(F(H)))                               # M_PI * 2 / static_cast<float>(H): double
        vres = F(float((F(top_angle) - F(btm_angle)) / F(V) / F(180.0)) * np.pi)
        btm_rad = float(F(btm_angle) / F(180.0)) * np.pi                # btm_angle_ / 180.f * M_PI: double
        vr = angle_f(z, dxy)
        row = trunc_x86((vr.astype(np.float64) - btm_rad) / float(vres))
        hr = angle_f(y, x)
        hr = np.where(hr < 0, (hr.astype(np.float64) + np.pi * 2).astype(F), hr).astype(F)
        q = (hr / hres).astype(F).astype(np.float64)
        col = np.where(q >= 0, np.floor(q + 0.5), np.ceil(q - 0.5))     # std::lround
        col = np.where(np.isfinite(col), col, 0).astype(np.int64)
    col = np.where(col >= H, col - H, col)
    ok = fin & ~(dxy < F(0.01)) & (row >= 0) & (row < V) & (col >= 0) & (col < H)
    return np.where(ok, row * H + col, -1)


def range_image(pts: np.ndarray, **kw) -> np.ndarray:
    """keep mask: the first row of every pixel, in input order"""
    pix = range_image_pixels(pts, **kw)
    keep = np.zeros(len(pix), bool)
    ids = np.flatnonzero(pix >= 0)
    _, first = np.unique(pix[ids], return_index=True)
    keep[ids[first]] = True
    return keep


# ---- chains --------------------------------------------------------------------------------------------------------------
def keep_mask(f: dict, pts: np.ndarray) -> np.ndarray:
    """one new filter, given as dict(type=..., <reference parameter names>)"""
    kw = {k: v for k, v in f.items() if k != "type"}
    if f["type"] == GROUND_REMOVAL:
        return ground_removal(pts, **kw)
    if f["type"] == GROUND_REMOVAL2:
        return ground_removal2(pts, **kw)
    if f["type"] == RANGE_IMAGE:
        return range_image(pts, **kw)
    raise ValueError(f["type"])


def run_chain(points5: np.ndarray, chain: list) -> tuple:
    """Factory::Filter over filters of both kinds: the three here and oracle/filters.py's five.
    Returns (filtered [M,5] float32, source_index [M] int32; -1 after a VoxelGrid)."""
    pts = np.asarray(points5, dtype=F)
    src = np.arange(len(pts), dtype=np.int32)
    for f in chain:
        if len(pts) == 0:
            break
        if f["type"] in (GROUND_REMOVAL, GROUND_REMOVAL2, RANGE_IMAGE):
            m = keep_mask(f, pts)
            pts, src = pts[m], src[m]
        else:
            if not of.config_valid(f):
                raise ValueError(f"ConfigsValid() is false for {f}")
            if f["type"] == of.VOXEL_GRID:
                pts = of.voxel_grid(pts, f["voxel_size"])
                src = np.full(len(pts), -1, dtype=np.int32)
            else:
                m = of.keep_mask(f, pts)
                pts, src = pts[m], src[m]
    return pts, src
