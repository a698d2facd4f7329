"""Python view of the map package (the reference's builder/map_package.{h,cc}, SaveTrajectoriesAsMapPackage): the static map cut
into overlapping square pieces, one PCD file per piece centred on the piece and an XML file that lists them.  include/smhip/
map_package.h is the C++ form and says what differs from the reference; both drive the same calls of libsmhip.so -- the plan
(smhip_map_package_plan, host only), the clipped insert, the clipped and recentred output, the clear -- and write the same bytes."""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass, field

import numpy as np

from . import _capi
from . import pcd as _pcd
from .matcher import SmhipError


@dataclass
class MapPackageOptions:                      # builder/map_package.h:36-41
    enable: bool = True
    border_offset: float = 100.0
    piece_width: float = 500.0
    cloud_file_prefix: str = "part_"
    descript_filename: str = "map_package.xml"


@dataclass
class Plan:
    x_steps: int
    y_steps: int
    centres: np.ndarray                       # [P, 2] float64, piece (x, y) at x * y_steps + y
    bb_min: np.ndarray                        # [P, 2]
    bb_max: np.ndarray                        # [P, 2]
    members: list = field(default_factory=list)   # per piece: int32 array of submap indices, ascending


def plan(translations, options: MapPackageOptions | None = None) -> Plan:
    """map_package.cc:59-141 on the host (no device): translations [n, 3] (or [n, 2]) float64, the submaps' global translations in
    trajectory order.  Raises SmhipError with the reason when the package is refused."""
    o = options or MapPackageOptions()
    lib = _capi.load_library()
    t = np.asarray(translations, dtype=np.float64)
    if t.ndim != 2 or t.shape[1] not in (2, 3):
        raise ValueError("translations must be [n, 2|3]")
    if t.shape[1] == 2:
        t = np.concatenate([t, np.zeros((len(t), 1))], axis=1)
    t = np.ascontiguousarray(t)
    co = _capi.MapPackageOptions()
    lib.smhip_map_package_default_options(ctypes.byref(co))
    co.border_offset, co.piece_width = float(o.border_offset), float(o.piece_width)
    steps = np.zeros(2, np.int32)
    n_members = ctypes.c_int32()
    why = ctypes.create_string_buffer(160)
    tp = t.ctypes.data_as(_capi.c_double_p) if len(t) else None
    st = lib.smhip_map_package_plan(len(t), tp, ctypes.byref(co), steps.ctypes.data_as(_capi.c_int32_p), 0, None, None, None, 0, None,
                                    ctypes.byref(n_members), why, len(why))
    if st != 0:
        raise SmhipError(st, why.value.decode())
    P = int(steps[0]) * int(steps[1])
    centres = np.zeros((P, 2)); boxes = np.zeros((P, 4)); offsets = np.zeros(P + 1, np.int32); members = np.zeros(max(n_members.value, 1), np.int32)
    st = lib.smhip_map_package_plan(len(t), tp, ctypes.byref(co), steps.ctypes.data_as(_capi.c_int32_p), P, centres.ctypes.data_as(_capi.c_double_p),
                                    boxes.ctypes.data_as(_capi.c_double_p), offsets.ctypes.data_as(_capi.c_int32_p), len(members),
                                    members.ctypes.data_as(_capi.c_int32_p), ctypes.byref(n_members), why, len(why))
    if st != 0:
        raise SmhipError(st, why.value.decode())
    return Plan(int(steps[0]), int(steps[1]), centres, boxes[:, :2].copy(), boxes[:, 2:].copy(),
                [members[offsets[i]:offsets[i + 1]].copy() for i in range(P)])


def piece_file(options: MapPackageOptions, x: int, y: int) -> str:
    return f"{options.cloud_file_prefix}{x}_{y}.pcd"                      # map_package.cc:201-203


def _escaped(s: str) -> str:
    out = []
    for ch in s:
        if ch == "&":
            out.append("&amp;")
        elif ch == "<":
            out.append("&lt;")
        elif ch == ">":
            out.append("&gt;")
        elif ch == '"':
            out.append("&quot;")
        elif ord(ch) < 32 and ch != "\t":
            out.append("&#%d%d;" % (ord(ch) // 10, ord(ch) % 10))
        else:
            out.append(ch)
    return "".join(out)


def xml_text(p: Plan, options: MapPackageOptions | None = None) -> str:
    """The description file (map_package.cc:211-227) as pugixml 1.9 writes it with its defaults; doubles as "%.17g"."""
    o = options or MapPackageOptions()
    if not len(p.centres):
        return '<?xml version="1.0"?>\n<MapPackage />\n'
    lines = ['<?xml version="1.0"?>', "<MapPackage>"]
    for x in range(p.x_steps):
        for y in range(p.y_steps):
            c = p.centres[x * p.y_steps + y]
            lines.append('\t<Piece x="%.17g" y="%.17g" file="%s" />' % (c[0], c[1], _escaped(piece_file(o, x, y))))
    return "\n".join(lines + ["</MapPackage>"]) + "\n"


def write_xml(path: str, p: Plan, options: MapPackageOptions | None = None) -> None:
    with open(path, "wb") as f:
        f.write(xml_text(p, options).encode())


def save_map_package(submaps, export_path: str, options: MapPackageOptions | None = None, device: int = 0, intensity_scale: float = 1.0,
                     table_log2: int = 22, max_table_log2: int | None = None, output_average: bool = False, output_rgb: bool = False,
                     **mrvm_settings) -> dict:
    """SaveTrajectoriesAsMapPackage for one trajectory.  submaps: a list of (global_pose [4, 4], cloud [n, 5] float32 in the submap's own
    coordinates).  export_path is joined to the file names as it is (give it its trailing separator).  mrvm_settings: MrvmSettings
    fields (prob_threshold, high_resolution, ...).  Returns dict(plan, files, points, inserts, clipped_inserts).  When anything fails
    the files this call wrote are removed and the error is raised."""
    from .mrvm import MultiResolutionVoxelMapHip
    o = options or MapPackageOptions()
    poses = [np.asarray(P, dtype=np.float64) for P, _ in submaps]
    clouds = [np.ascontiguousarray(c, dtype=np.float32) for _, c in submaps]
    if any(c.ndim != 2 or c.shape[1] != 5 for c in clouds if len(c)):
        raise ValueError("a submap's cloud is [n, 5] float32 (InnerPointType rows)")
    pl = plan(np.array([P[:3, 3] for P in poses]).reshape(-1, 3), o)
    descript = export_path + o.descript_filename
    with open(descript, "wb"):                  # its place is taken first: a missing directory ends the call before any device work
        pass
    written = [descript]
    try:
        m = MultiResolutionVoxelMapHip(device=device, table_log2=min(table_log2, max_table_log2 or 28), max_cloud_points=max([len(c) for c in clouds] + [1]),
                                       max_table_log2=max_table_log2, **mrvm_settings)
        try:
            points = inserts = clipped = 0
            for i in range(len(pl.centres)):
                x, y = divmod(i, pl.y_steps)
                lo, hi, centre = pl.bb_min[i], pl.bb_max[i], pl.centres[i]
                if i > 0:
                    m.clear()
                for k in pl.members[i]:
                    if not len(clouds[k]):
                        continue
                    px, py = poses[k][0, 3], poses[k][1, 3]
                    if lo[0] <= px <= hi[0] and lo[1] <= py <= hi[1]:          # map_package.cc:162-166
                        m.insert_transformed(clouds[k], poses[k], intensity_scale)
                        inserts += 1
                    elif m.insert_transformed_clipped(clouds[k], poses[k], lo, hi, intensity_scale) > 0:   # :167-182
                        inserts += 1
                        clipped += 1
                rows = m.output_clipped(lo, hi, centre, average=output_average, rgb=output_rgb, packed_rgb=True)
                name = export_path + piece_file(o, x, y)
                written.append(name)
                with open(name, "wb") as f:
                    f.write(_pcd.header(len(rows), output_rgb))
                    f.write(np.ascontiguousarray(rows, np.float32).tobytes())
                points += len(rows)
        finally:
            m.close()
        write_xml(descript, pl, o)
    except BaseException:
        for name in written:
            if os.path.exists(name):
                os.remove(name)
        raise
    return dict(plan=pl, files=written[1:] + [descript], points=points, inserts=inserts, clipped_inserts=clipped)
