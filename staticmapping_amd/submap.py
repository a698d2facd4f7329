"""ctypes view of the device submap build (include/smhip.h, `smhip_submap_build_f32` / `smhip_filter_output_to_target`) and the
Python mirror of the bookkeeping of static_map::Submap (the reference's builder/submap.cc:76-163; include/smhip/submap.h is the
C++ form): frames are moved into the first frame's coordinates, concatenated, optionally passed through a VoxelGrid, and the
result goes through CalculateNormals -- all on the device, the cloud never returns to the host unless it is asked for."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _capi
from . import filters as _filters


def text_voxel_size(voxel_size: float) -> float:
    """The voxel size as the filter receives it: written with std::to_string (six decimals, submap.cc:148-154) and parsed back
    to float, as include/smhip/filters.h parses a float parameter."""
    return float(np.float32(float("%f" % float(np.float32(voxel_size)))))


def _launch(matcher, frames, local_poses, voxel_size, motions=None) -> int:
    arrs = [np.ascontiguousarray(np.asarray(f, dtype=np.float32)) for f in frames]
    strides = {a.shape[1] for a in arrs if a.ndim == 2}
    if any(a.ndim != 2 for a in arrs) or len(strides) > 1:
        raise ValueError("frames must be 2-d float32 arrays with one row width (4 = x y z intensity, 5 = InnerPointType)")
    k = len(arrs)
    stride = strides.pop() if strides else 0
    poses = np.ascontiguousarray([np.asarray(P, dtype=np.float64).T.reshape(16) for P in local_poses], dtype=np.float64).reshape(-1)
    if len(poses) != 16 * k:
        raise ValueError("one 4x4 local pose per frame")
    n = np.ascontiguousarray([len(a) for a in arrs], dtype=np.int32)
    rows = (_capi.c_float_p * max(1, k))(*[a.ctypes.data_as(_capi.c_float_p) for a in arrs])
    n_out = ctypes.c_int()
    if motions is None:
        matcher._check(matcher._lib.smhip_submap_build_f32(matcher._h, k, rows, stride, n.ctypes.data_as(_capi.c_int32_p),
                                                           poses.ctypes.data_as(_capi.c_double_p), float(voxel_size), ctypes.byref(n_out)))
        return n_out.value
    mot = np.ascontiguousarray([np.asarray(M, dtype=np.float64).T.reshape(16) for M in motions], dtype=np.float64).reshape(-1)
    if len(mot) != 16 * k:
        raise ValueError("one 4x4 sweep motion per frame")
    matcher._check(matcher._lib.smhip_submap_build_compensated_f32(matcher._h, k, rows, stride, n.ctypes.data_as(_capi.c_int32_p),
                                                                   poses.ctypes.data_as(_capi.c_double_p), mot.ctypes.data_as(_capi.c_double_p),
                                                                   float(voxel_size), ctypes.byref(n_out)))
    return n_out.value


def build_submap_resident(matcher, frames, local_poses, voxel_size: float = 0.0, motions=None) -> int:
    """Submap::InsertFrame's cloud for a full submap, left on the device as the filter workspace's current cloud; returns its
    size.  Follow with output_to_target() / filters.output_to_source() or read it with get_submap().  motions: one 4x4 per frame,
    the sensor's motion during that frame's sweep -- every frame is de-skewed by it before its local pose is applied
    (smhip_submap_build_compensated_f32)."""
    return _launch(matcher, frames, local_poses, voxel_size, motions)


def get_submap(matcher, n: int):
    """The resident cloud: (float32 [n, 5] InnerPointType rows, int32 [n] row of the concatenated input or -1 after the voxel filter)."""
    out = np.zeros((n, 5), np.float32)
    src = np.zeros(n, np.int32)
    matcher._check(matcher._lib.smhip_filter_get_output(matcher._h, out.ctypes.data_as(_capi.c_float_p),
                                                        src.ctypes.data_as(_capi.c_int32_p), n))
    return out, src


def build_submap(matcher, frames, local_poses, voxel_size: float = 0.0, motions=None):
    """frames: float32 [n_k, 4] (KITTI rows; factor = i / n_k) or [n_k, 5] arrays; local_poses: one 4x4 per frame (frame ->
    first frame); voxel_size 0 = enable_voxel_filter false; motions: as build_submap_resident.  Returns (cloud [M, 5] float32,
    source_index [M] int32)."""
    return get_submap(matcher, _launch(matcher, frames, local_poses, voxel_size, motions))


def output_to_target(matcher, slot: int = 0) -> int:
    """Device CalculateNormals of the resident cloud into the target of `slot` (submap.cc:160-161); returns the target's size."""
    m = ctypes.c_int()
    matcher._check(matcher._lib.smhip_filter_output_to_target(matcher._h, slot, ctypes.byref(m)))
    return m.value


output_to_source = _filters.output_to_source


class SubmapBuilder:
    """The bookkeeping of static_map::Submap: InsertFrame until `frame_count` frames are in (submap.cc:76-96), then the cloud
    (:98-161).  Options and defaults: builder/submap_options.h (frame_count 5, enable_voxel_filter false, voxel_size 0.1)."""

    def __init__(self, frame_count: int = 5, enable_voxel_filter: bool = False, voxel_size: float = 0.1):
        self.frame_count, self.enable_voxel_filter, self.voxel_size = int(frame_count), bool(enable_voxel_filter), float(voxel_size)
        self.frames, self.local_poses = [], []
        self.global_pose = None
        self.motions = None                                               # set_motions: the frames are de-skewed when the cloud is built

    def full(self) -> bool:
        return len(self.frames) == self.frame_count

    def insert_frame(self, cloud, global_pose):
        if self.full():
            raise RuntimeError("InsertFrame on a full submap (CHECK(!full_), submap.cc:78)")
        P = np.asarray(global_pose, dtype=np.float64)
        if not self.frames:
            self.global_pose = P.copy()                                   # :83-84
            self.local_poses.append(np.eye(4))
        else:
            self.local_poses.append(np.linalg.inv(self.global_pose) @ P)  # :87
        self.frames.append(np.ascontiguousarray(np.asarray(cloud, dtype=np.float32)))

    def set_motions(self, motions):
        """One 4x4 per frame, the sensor's motion during that frame's sweep (None: no compensation)."""
        self.motions = None if motions is None else [np.asarray(M, dtype=np.float64) for M in motions]

    def first_frame_pose(self):
        return self.global_pose

    def local_pose(self, i: int):
        return self.local_poses[i]

    def device_voxel_size(self) -> float:
        return text_voxel_size(self.voxel_size) if self.enable_voxel_filter else 0.0

    def build_resident(self, matcher) -> int:
        if not self.full():
            raise RuntimeError("the submap is not full: it has no cloud yet")
        return build_submap_resident(matcher, self.frames, self.local_poses, self.device_voxel_size(), self.motions)

    def cloud(self, matcher):
        """Submap::Cloud() without its normals: (rows [M, 5], source_index [M])."""
        return get_submap(matcher, self.build_resident(matcher))

    def to_target(self, matcher, slot: int = 0) -> int:
        self.build_resident(matcher)
        return output_to_target(matcher, slot)

    def to_source(self, matcher, slot: int = 0) -> int:
        n = self.build_resident(matcher)
        output_to_source(matcher, slot)
        return n
