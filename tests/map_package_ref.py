"""SaveTrajectoriesAsMapPackage restated in numpy, line by line, from the reference's builder/map_package.cc (cited as :N below;
options and defaults builder/map_package.h:36-41).  This is the text the device path is tested against: the plan in Python floats
(IEEE doubles, as the reference's), the point tests on float32 coordinates widened to float64, the voxel map itself behind any
object with insert(points5, origin) and dump() -- the tests hand in oracle.cref.Mrvm.

  plan()          :59-141   extent, step counts, centres, boxes, members
  fill_piece()    :143-184  whole or clipped insert of every member submap
  cut()           :186-198  rows inside the box, moved to the centre
  xml_text()      :210-227  the description as the vendored pugixml 1.9 writes it (third_parties/pugixml/pugixml.cc:4668 "%.17g",
                            :4090-4122 element layout, :7160-7163 declaration)
"""
import numpy as np

DEFAULTS = dict(border_offset=100.0, piece_width=500.0, cloud_file_prefix="part_", descript_filename="map_package.xml")   # map_package.h:36-41


class Refused(Exception):
    """The reference returns false and saves no package (:92-95)."""


def clamp(v, lo, hi):                                     # common::Clamp, common/math.h:66-75
    return hi if v > hi else (lo if v < lo else v)


def inside_bbox(px, py, bb_min, bb_max):                  # :110-115, closed on every side
    return bool(px >= bb_min[0] and px <= bb_max[0] and py >= bb_min[1] and py <= bb_max[1])


def plan(translations, border_offset=100.0, piece_width=500.0):
    """translations: the submaps' GlobalTranslation in trajectory order.  Returns dict(x_steps, y_steps, pieces) with pieces x-major,
    each dict(x, y, centre, bb_min, bb_max, members)."""
    t = [(float(p[0]), float(p[1])) for p in translations]
    min_x, max_x, min_y, max_y = 1.e50, -1.e50, 1.e50, -1.e50                     # :60-63
    for px, py in t:                                                             # :64-81
        if px > max_x:
            max_x = px
        if px < min_x:
            min_x = px
        if py > max_y:
            max_y = py
        if py < min_y:
            min_y = py
    border_offset, piece_width = float(border_offset), float(piece_width)
    min_x -= border_offset; min_y -= border_offset; max_x += border_offset; max_y += border_offset   # :83-86
    half_width = piece_width * 0.5                                               # :89
    x_steps = int((max_x - min_x) / half_width)                                  # :90-91: double -> int truncates toward zero, as int() does
    y_steps = int((max_y - min_y) / half_width)
    if x_steps < 0 or y_steps < 0:                                               # :92-95
        raise Refused("No good bounding box, save no map package.")
    if x_steps == 0:                                                             # :103-108
        x_steps += 1
    if y_steps == 0:
        y_steps += 1
    pieces = []
    for x in range(x_steps):                                                     # :119-141
        for y in range(y_steps):
            centre = (min_x + (x + 1) * half_width, min_y + (y + 1) * half_width)                    # :122
            bb_min = [centre[0] - half_width, centre[1] - half_width]                                # :123
            bb_max = [centre[0] + half_width, centre[1] + half_width]                                # :124
            bb_min[0] = clamp(bb_min[0], min_x, max_x); bb_max[0] = clamp(bb_max[0], min_x, max_x)   # :125-126
            bb_min[1] = clamp(bb_min[1], min_y, max_y); bb_max[1] = clamp(bb_max[1], min_y, max_y)   # :127-128
            lo = (bb_min[0] - border_offset, bb_min[1] - border_offset)                              # :130
            hi = (bb_max[0] + border_offset, bb_max[1] + border_offset)                              # :131
            members = [i for i, (px, py) in enumerate(t) if inside_bbox(px, py, lo, hi)]             # :132-139
            pieces.append(dict(x=x, y=y, centre=centre, bb_min=tuple(bb_min), bb_max=tuple(bb_max), members=members))
    return dict(x_steps=x_steps, y_steps=y_steps, pieces=pieces)


def transform_rows(rows5, pose, scale=1.0):
    """ApplyTransformToOutput(pose) (:157-158) through TransformPoint (builder/data/cloud_types.cc:167-178): the pose cast to float,
    ((m00 x + m01 y) + m02 z) + m03 with every product and sum rounded to float.  scale: what the device path multiplies the
    intensity by (1 for clouds that already carry the reader's intensities)."""
    m = np.asarray(pose, dtype=np.float64).astype(np.float32)
    p = np.asarray(rows5, dtype=np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.zeros((len(p), 5), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(3):
            out[:, i] = ((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3]
        out[:, 3] = p[:, 3] * np.float32(scale)
    if p.shape[1] > 4:
        out[:, 4] = p[:, 4]
    return out


def rows_in_box(rows, bb_min, bb_max):
    """:171-176 and :191-193: inside_bbox(Eigen::Vector3d(point.x, point.y, point.z), ...) -- the float coordinates widened to double,
    closed comparisons, so a NaN coordinate is outside."""
    x = np.asarray(rows)[:, 0].astype(np.float64)
    y = np.asarray(rows)[:, 1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (x >= bb_min[0]) & (x <= bb_max[0]) & (y >= bb_min[1]) & (y <= bb_max[1])


def member_rows(cloud5, pose, piece, scale=1.0):
    """The rows one member submap inserts into a piece's map, and whether it went in whole (:153-182).  None: no insert at all."""
    pose = np.asarray(pose, dtype=np.float64)
    world = transform_rows(cloud5, pose, scale)
    if inside_bbox(pose[0, 3], pose[1, 3], piece["bb_min"], piece["bb_max"]):    # :162
        return world, True
    kept = world[rows_in_box(world, piece["bb_min"], piece["bb_max"])]           # :171-176, in their order
    return (kept, False) if len(kept) else (None, False)                        # :177


def fill_piece(voxel_map, submaps, piece, scale=1.0):
    """submaps: [(pose, cloud5)].  Every member in order; origin = translation.cast<float>() (:164-165, 178-179).  An empty cloud makes
    no insert (InsertPointCloud returns at once, multi_resolution_voxel_map.cc:61-64).  Returns (whole, clipped, skipped) counts."""
    counts = [0, 0, 0]
    for k in piece["members"]:
        pose, cloud = submaps[k]
        if not len(cloud):
            counts[2] += 1
            continue
        rows, whole = member_rows(cloud, pose, piece, scale)
        if rows is None:
            counts[2] += 1
            continue
        voxel_map.insert(rows, np.asarray(pose, np.float64)[:3, 3].astype(np.float32))
        counts[0 if whole else 1] += 1
    return tuple(counts)


def sorted_output(voxel_map, threshold=0.6, average=False, rgb=False, use_max_intensity=True):
    """OutputToPointCloud (multi_resolution_voxel_map.cc:125-216) with the rows in voxel-key order (x, then y, then z; stored-point
    order within a voxel), from the map's dump.  rgb: the 4th column is the grey level min(255, uint32(max_intensity * 1.4))."""
    keys, prob, mi, npts, pts = voxel_map.dump()                                 # sorted by key
    thr = int(np.float32(threshold) * np.float32(256))                           # static_cast<uint8_t>(threshold * kTableSize), .cc:132
    keep = (prob >= thr) & (npts > 0)
    mi, npts, pts = mi[keep], npts[keep], pts[keep]
    grey = np.minimum(255, (mi.astype(np.float64) * 1.4).astype(np.uint32)).astype(np.float32)
    if average:
        acc = np.zeros((len(npts), 3), np.float32)
        for k in range(pts.shape[1]):
            acc = np.where((k < npts)[:, None], acc + pts[:, k, :3], acc).astype(np.float32)
        out = np.zeros((len(npts), 4), np.float32)
        out[:, :3] = acc / npts.astype(np.float32)[:, None]
        out[:, 3] = grey if rgb else (mi.astype(np.float32) if use_max_intensity else 0.0)
        return out
    v = np.repeat(np.arange(len(npts)), npts)
    k = np.arange(len(v)) - np.repeat(np.cumsum(npts) - npts, npts)
    out = np.zeros((len(v), 4), np.float32)
    out[:, :3] = pts[v, k, :3]
    out[:, 3] = grey[v] if rgb else (mi[v].astype(np.float32) if use_max_intensity else pts[v, k, 3])
    return out


def cut(rows, bb_min, bb_max, centre):
    """:191-198: the rows inside the box; point.x -= part.center[0] is float -= double, computed in double and rounded to float once."""
    r = np.asarray(rows, np.float32)
    r = r[rows_in_box(r, bb_min, bb_max)].copy()
    r[:, 0] = (r[:, 0].astype(np.float64) - centre[0]).astype(np.float32)
    r[:, 1] = (r[:, 1].astype(np.float64) - centre[1]).astype(np.float32)
    return r


def piece_file(prefix, x, y):
    return "%s%d_%d.pcd" % (prefix, x, y)                                        # :201-203


def xml_text(pl, prefix="part_"):
    lines = ['<?xml version="1.0"?>', "<MapPackage>"]
    for p in pl["pieces"]:                                                       # x-major, :213-225
        lines.append('\t<Piece x="%.17g" y="%.17g" file="%s" />' % (p["centre"][0], p["centre"][1], piece_file(prefix, p["x"], p["y"])))
    return "\n".join(lines + ["</MapPackage>"]) + "\n"


def package(submaps, make_map, border_offset=100.0, piece_width=500.0, prefix="part_", scale=1.0, threshold=0.6, average=False, rgb=False):
    """The whole of :51-230: {file name: rows [n, 4] float32} and the plan.  make_map() returns a fresh voxel map (Initialise, :149-150)."""
    pl = plan([np.asarray(P, np.float64)[:3, 3] for P, _ in submaps], border_offset, piece_width)
    files, stats = {}, []
    for p in pl["pieces"]:
        m = make_map()
        stats.append(fill_piece(m, submaps, p, scale))
        files[piece_file(prefix, p["x"], p["y"])] = cut(sorted_output(m, threshold, average, rgb), p["bb_min"], p["bb_max"], p["centre"])
        if hasattr(m, "close"):
            m.close()
    return files, pl, stats


# ---- not the reference's: the double arithmetic smhip_shard makes a submap's local poses with, restated operation by operation so
# that a test can build the very clouds the driver builds (csrc/shard_poses.h AffineInverse, MulPose; 4x4 numpy arrays in and out)
def affine_inverse(P):
    m = [[float(P[r][c]) for c in range(4)] for r in range(4)]
    c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1]
    c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2]
    c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0]
    det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02
    inv = [[c00 / det, (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det, (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det],
           [c01 / det, (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det, (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det],
           [c02 / det, (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det, (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det]]
    out = np.zeros((4, 4))
    for r in range(3):
        for c in range(3):
            out[r, c] = inv[r][c]
        out[r, 3] = -(inv[r][0] * m[0][3] + inv[r][1] * m[1][3] + inv[r][2] * m[2][3])
    out[3, 3] = 1.0
    return out


def mul_pose(A, B):
    out = np.zeros((4, 4))
    for r in range(4):
        for c in range(4):
            s = 0.0
            for k in range(4):
                s += float(A[r][k]) * float(B[k][c])
            out[r, c] = s
    return out


def submap_local_poses(frame_poses):
    """local pose = first^-1 * frame (builder/submap.cc:83-87), the first the identity."""
    first_inv = affine_inverse(frame_poses[0])
    return [np.eye(4)] + [mul_pose(first_inv, P) for P in frame_poses[1:]]
