"""Python view of static_map::MultiResolutionVoxelMap on the GPU (/root/reference/builder/multi_resolution_voxel_map.{h,cc}):
Initialise (constructor) / insert_point_cloud / output_to_point_cloud, all compute inside libsmhip.so."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi
from .matcher import SmhipError


class MultiResolutionVoxelMapHip:
    def __init__(self, device: int = 0, table_log2: int = 22, max_cloud_points: int = 262144, max_table_log2: int | None = None, **settings):
        """table_log2: the table's FIRST size; it doubles between inserts as the map grows, up to 2^max_table_log2 (default 28)."""
        self._lib = _capi.load_library()
        self.settings = _capi.MrvmSettings()
        self._lib.smhip_mrvm_default_settings(ctypes.byref(self.settings))
        for k, v in settings.items():
            if not hasattr(self.settings, k):
                raise KeyError(f"unknown MRVM setting {k}")
            setattr(self.settings, k, v)
        self._h = ctypes.c_void_p()
        st = self._lib.smhip_mrvm_create(device, table_log2, max_cloud_points, ctypes.byref(self.settings), ctypes.byref(self._h))
        if st != 0:
            self._h = ctypes.c_void_p()
            raise SmhipError(st, self._lib.smhip_status_string(st).decode())
        self.last_warning = ""
        self.last_skipped = 0
        if max_table_log2 is not None:
            self._check(self._lib.smhip_mrvm_set_max_table_log2(self._h, max_table_log2))

    @property
    def table_log2(self) -> int:
        return int(self._lib.smhip_mrvm_table_log2(self._h))

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.smhip_mrvm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != 0:
            raise SmhipError(st, self._lib.smhip_mrvm_last_error(self._h).decode())

    def insert_point_cloud(self, points, origin):
        """points [N, 4+] float32 rows x y z intensity [factor] in the map frame; origin = the frame's sensor position."""
        p = np.ascontiguousarray(points, dtype=np.float32)
        o = np.ascontiguousarray(origin, dtype=np.float32)
        self._check(self._lib.smhip_mrvm_insert_f32(self._h, p.ctypes.data_as(_capi.c_float_p), p.shape[1], p.shape[0], o.ctypes.data_as(_capi.c_float_p)))
        # applied; what the device had to say about it (points beyond +-2^20 voxels skipped, table filling up) -- "" if nothing
        self.last_warning = self._lib.smhip_mrvm_last_error(self._h).decode()
        n = ctypes.c_int32()
        self._lib.smhip_mrvm_last_skipped(self._h, ctypes.byref(n))
        self.last_skipped = n.value

    def insert_transformed(self, rows, pose, intensity_scale: float = 1.0):
        """ApplyTransformToOutput(pose) + InsertPointCloud (map_builder.cc:842-848), the transform on the device: rows [N, 4] (KITTI
        x y z reflectance; factor 0) or [N, 5] (InnerPointType) in the sensor frame, pose [4, 4] (row-major numpy) sensor -> map.
        The reference's TransformPoint: the pose cast to float, every product and sum rounded to float; origin = the pose's
        translation cast to float; intensity = row[3] * intensity_scale in float (255 for raw KITTI rows, kitti_reader.cc:113)."""
        p = np.ascontiguousarray(rows, dtype=np.float32)
        T = np.asarray(pose, dtype=np.float64)
        if p.ndim != 2 or T.shape != (4, 4):
            raise ValueError("rows must be [N, 4|5], pose [4, 4]")
        cm = np.ascontiguousarray(T.T).ravel()                    # column-major, as everywhere in the ABI
        self._check(self._lib.smhip_mrvm_insert_transformed_f32(self._h, p.ctypes.data_as(_capi.c_float_p), p.shape[1], p.shape[0],
                                                                cm.ctypes.data_as(_capi.c_double_p), float(intensity_scale)))
        self.last_warning = self._lib.smhip_mrvm_last_error(self._h).decode()
        n = ctypes.c_int32()
        self._lib.smhip_mrvm_last_skipped(self._h, ctypes.byref(n))
        self.last_skipped = n.value

    def insert_compensated(self, rows, pose, motion, intensity_scale: float = 1.0):
        """insert_transformed of the frame de-skewed by `motion` [4, 4], the sensor's motion during its sweep (inv(pose) @ the next
        frame's pose), `pose` being the sensor pose at the start of the sweep: MotionCompensation (map_builder.cc:232-257) per row,
        the coordinates rounded to float, then TransformPoint -- one kernel, the de-skewed cloud is never stored.  The factor is
        rows[:, 4], or float32(i / N) for [N, 4] rows, and is stored with the point.  A factor outside [0, 1] or NaN raises and
        leaves the map bit for bit as it was."""
        p = np.ascontiguousarray(rows, dtype=np.float32)
        T = np.asarray(pose, dtype=np.float64)
        M = np.asarray(motion, dtype=np.float64)
        if p.ndim != 2 or T.shape != (4, 4) or M.shape != (4, 4):
            raise ValueError("rows must be [N, 4|5], pose and motion [4, 4]")
        cm = np.ascontiguousarray(T.T).ravel()
        mm = np.ascontiguousarray(M.T).ravel()
        self._check(self._lib.smhip_mrvm_insert_compensated_f32(self._h, p.ctypes.data_as(_capi.c_float_p), p.shape[1], p.shape[0],
                                                                cm.ctypes.data_as(_capi.c_double_p), mm.ctypes.data_as(_capi.c_double_p),
                                                                float(intensity_scale)))
        self.last_warning = self._lib.smhip_mrvm_last_error(self._h).decode()
        n = ctypes.c_int32()
        self._lib.smhip_mrvm_last_skipped(self._h, ctypes.byref(n))
        self.last_skipped = n.value

    def insert_transformed_clipped(self, rows, pose, bb_min, bb_max, intensity_scale: float = 1.0) -> int:
        """insert_transformed of the rows whose transformed x, y lie in the closed box [bb_min, bb_max] (builder/map_package.cc:169-179;
        float coordinates against double bounds, a NaN fails), in their order.  Returns the number of rows kept; with none the map is
        left exactly as it was."""
        p = np.ascontiguousarray(rows, dtype=np.float32)
        T = np.asarray(pose, dtype=np.float64)
        if p.ndim != 2 or T.shape != (4, 4):
            raise ValueError("rows must be [N, 4|5], pose [4, 4]")
        cm = np.ascontiguousarray(T.T).ravel()
        lo = np.ascontiguousarray(bb_min, dtype=np.float64).reshape(2)
        hi = np.ascontiguousarray(bb_max, dtype=np.float64).reshape(2)
        kept = ctypes.c_int32()
        self._check(self._lib.smhip_mrvm_insert_transformed_clipped_f32(self._h, p.ctypes.data_as(_capi.c_float_p), p.shape[1], p.shape[0],
                                                                        cm.ctypes.data_as(_capi.c_double_p), float(intensity_scale),
                                                                        lo.ctypes.data_as(_capi.c_double_p), hi.ctypes.data_as(_capi.c_double_p),
                                                                        ctypes.byref(kept)))
        self.last_warning = self._lib.smhip_mrvm_last_error(self._h).decode()
        n = ctypes.c_int32()
        self._lib.smhip_mrvm_last_skipped(self._h, ctypes.byref(n))
        self.last_skipped = n.value
        return kept.value

    def output_clipped(self, bb_min, bb_max, centre, threshold: float | None = None, average: bool = False, rgb: bool = False,
                       packed_rgb: bool = False, count_only: bool = False):
        """The sorted output's rows inside the closed box, moved to `centre`: x <- float32(float64(x) - centre[0]), the same for y
        (builder/map_package.cc:191-197).  With average the averaged row is tested.  count_only: the number of rows, nothing written."""
        thr = self.settings.prob_threshold if threshold is None else threshold
        flags = (1 if average else 0) | (2 if rgb else 0)
        lo, hi, c = (np.ascontiguousarray(v, dtype=np.float64).reshape(2) for v in (bb_min, bb_max, centre))
        args = (lo.ctypes.data_as(_capi.c_double_p), hi.ctypes.data_as(_capi.c_double_p), c.ctypes.data_as(_capi.c_double_p))
        n = ctypes.c_int32()
        self._check(self._lib.smhip_mrvm_output_clipped(self._h, thr, flags, *args, None, 0, ctypes.byref(n)))
        if count_only:
            return n.value
        out = np.zeros((max(n.value, 1), 4), np.float32)
        self._check(self._lib.smhip_mrvm_output_clipped(self._h, thr, flags, *args, out.ctypes.data_as(_capi.c_float_p), len(out), ctypes.byref(n)))
        out = out[:n.value]
        if rgb and not packed_rgb:
            out[:, 3] = (out[:, 3].copy().view(np.uint32) & 0xff).astype(np.float32)
        return out

    def clear(self):
        """Empties the map on the device; the table keeps its current size."""
        self._check(self._lib.smhip_mrvm_clear(self._h))
        self.last_warning = ""
        self.last_skipped = 0

    def voxel_count(self) -> int:
        n = ctypes.c_int32()
        self._check(self._lib.smhip_mrvm_voxel_count(self._h, ctypes.byref(n)))
        return n.value

    def output_to_point_cloud(self, threshold: float | None = None, average: bool = False, rgb: bool = False, sorted: bool = False,
                              packed_rgb: bool = False) -> np.ndarray:
        """OutputToPointCloud (multi_resolution_voxel_map.cc:125-216): rows x y z intensity; average = MrvmSettings::output_average
        (one mean point per voxel); rgb = the PointXYZRGB overload, 4th column = the grey level 0..255 (the packed colour's byte), or
        with packed_rgb the packed colour's bits as PCL's `rgb` float (what pcd.write_pcd(..., rgb=True) expects).  sorted: rows in
        voxel-key order (x, then y, then z of the voxel), stored-point order within a voxel -- ordered on the device, the same map
        gives the same array every time; otherwise table order."""
        thr = self.settings.prob_threshold if threshold is None else threshold
        flags = (1 if average else 0) | (2 if rgb else 0) | (4 if sorted else 0)
        n = ctypes.c_int32()
        self._check(self._lib.smhip_mrvm_output_ex(self._h, thr, flags, None, 0, ctypes.byref(n)))
        out = np.zeros((max(n.value, 1), 4), np.float32)
        self._check(self._lib.smhip_mrvm_output_ex(self._h, thr, flags, out.ctypes.data_as(_capi.c_float_p), len(out), ctypes.byref(n)))
        out = out[:n.value]
        if rgb and not packed_rgb:                # packed r << 16 | g << 8 | b in the float's bits, r = g = b
            out[:, 3] = (out[:, 3].copy().view(np.uint32) & 0xff).astype(np.float32)
        return out

    def dump(self):
        """(keys [V,3], prob [V], max_intensity [V], npoints [V], points [V, max, 5]) sorted by key -- the parity tests' view."""
        V = max(self.voxel_count(), 1)
        P = self.settings.max_point_num_in_cell
        keys = np.zeros((V, 3), np.int32); prob = np.zeros(V, np.uint8); mi = np.zeros(V, np.int32); npts = np.zeros(V, np.int32)
        pts = np.zeros((V, P, 5), np.float32)
        n = ctypes.c_int32()
        self._check(self._lib.smhip_mrvm_dump(self._h, keys.ctypes.data_as(_capi.c_int32_p), prob.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                              mi.ctypes.data_as(_capi.c_int32_p), npts.ctypes.data_as(_capi.c_int32_p), pts.ctypes.data_as(_capi.c_float_p),
                                              V, ctypes.byref(n)))
        keys, prob, mi, npts, pts = keys[:n.value], prob[:n.value], mi[:n.value], npts[:n.value], pts[:n.value]
        o = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
        return keys[o], prob[o], mi[o], npts[o], pts[o]
