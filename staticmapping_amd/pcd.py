"""The static map's file format: the PCD files pcl::io::savePCDFileBinary writes for PointXYZI / PointXYZRGB clouds (PCL 1.8;
MultiResolutionVoxelMap::OutputToPointCloud, builder/multi_resolution_voxel_map.cc:217-242), byte for byte what
include/smhip/pcd.h writes.  An 11-line v0.7 header ending in `DATA binary`, then n packed rows of four float32.  For XYZRGB the
fourth field is `rgb`, a float holding the packed colour's bits.  `binary_compressed` is not written."""
from __future__ import annotations

import sys

import numpy as np


def header(n: int, rgb: bool = False) -> bytes:
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z " + ("rgb" if rgb else "intensity") +
            f"\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH {n}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {n}\nDATA binary\n").encode()


def pack_grey(grey) -> np.ndarray:
    """Grey levels 0..255 -> PCL's packed `rgb` float (a = 255, r = g = b = grey), as the device writes it."""
    g = np.asarray(grey).astype(np.uint32) & 0xff
    return (np.uint32(0xff000000) | (g << 16) | (g << 8) | g).astype(np.uint32).view(np.float32)


def write_pcd(path: str, rows, rgb: bool = False) -> bool:
    """rows [n, 4] float32 (x y z intensity, or x y z packed rgb).  An empty cloud writes no file (False), with the reference's
    warning (:226-228)."""
    r = np.ascontiguousarray(rows, dtype=np.float32)
    if r.size == 0:
        print("[WARNING] Cloud is empty. Do not output to file.", file=sys.stderr)
        return False
    if r.ndim != 2 or r.shape[1] != 4:
        raise ValueError("rows must be [n, 4]")
    with open(path, "wb") as f:
        f.write(header(len(r), rgb))
        f.write(r.tobytes())
    return True


def read_pcd(path: str):
    """(rows [n, 4] float32, fields) of a binary PCD file with four 4-byte F fields (what write_pcd writes)."""
    with open(path, "rb") as f:
        data = f.read()
    meta, pos = {}, 0
    while True:
        end = data.index(b"\n", pos)
        line = data[pos:end].decode("ascii")
        pos = end + 1
        if line.startswith("#"):
            continue
        key, _, val = line.partition(" ")
        meta[key] = val.split()
        if key == "DATA":
            break
    fields = meta["FIELDS"]
    if meta["DATA"] != ["binary"] or meta["SIZE"] != ["4"] * 4 or meta["TYPE"] != ["F"] * 4 or meta.get("COUNT", ["1"] * 4) != ["1"] * 4:
        raise ValueError(f"unsupported PCD layout: {meta}")
    n = int(meta["POINTS"][0])
    rows = np.frombuffer(data, dtype=np.float32, count=4 * n, offset=pos).reshape(n, 4).copy()
    if pos + 16 * n != len(data):
        raise ValueError(f"{path}: {len(data) - pos} data bytes for {n} points")
    return rows, fields
