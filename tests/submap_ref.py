"""Submap::InsertFrame's cloud for a full submap (the reference's builder/submap.cc:98-158) restated in numpy -- what the device
build (smhip_submap_build_f32) is compared with, bit for bit.  CPU only.

  submap.cc:116-119  every frame goes through ApplyTransformToOutput(frame->LocalPose()): TransformPoint per point
                     (builder/data/cloud_types.cc:167-178, restated in tests/test_transform_point.py); intensity and factor are
                     carried unchanged
  submap.cc:123      *added_cloud += *transformed_cloud: the frames are concatenated in frame order
  submap.cc:144-158  with enable_voxel_filter: a VoxelGrid of voxel_size over the sum (oracle.filters.voxel_grid: double sums per
                     voxel in arrival order, output sorted by voxel index); the size travels through std::to_string, :151
  data_collector.h:202-204  rows of 4 floats get the collector's factor i / size of their own frame (oracle.filters.with_factor)
"""
import numpy as np

from oracle import filters as of
from test_transform_point import transform_point_f32


def text_voxel_size(voxel_size):
    """std::to_string(float) (six decimals, submap.cc:151) read back as the filter's float parameter."""
    return float(np.float32(float("%f" % float(np.float32(voxel_size)))))


def concatenate(frames, local_poses):
    """The sum of the transformed frames: float32 [sum n, 5] InnerPointType rows."""
    parts = []
    for rows, pose in zip(frames, local_poses):
        r = np.asarray(rows, dtype=np.float32)
        r5 = of.with_factor(r) if r.shape[1] == 4 else r[:, :5].copy()
        if len(r5):
            r5[:, :3] = transform_point_f32(r5, pose)
        parts.append(r5.reshape(-1, 5))
    return np.concatenate(parts).astype(np.float32)


def build_submap(frames, local_poses, voxel_size=0.0):
    """(cloud [M, 5] float32, source_index [M] int32): the row of the concatenation, or -1 after the voxel filter."""
    cloud = concatenate(frames, local_poses)
    if voxel_size > 0 and len(cloud):
        out = of.voxel_grid(cloud, voxel_size)
        return out, np.full(len(out), -1, dtype=np.int32)
    return cloud, np.arange(len(cloud), dtype=np.int32)


def local_poses(global_poses):
    """submap.cc:83-87: identity for the first frame, first^-1 * pose for the others."""
    first = np.asarray(global_poses[0], dtype=np.float64)
    return [np.eye(4)] + [np.linalg.inv(first) @ np.asarray(P, dtype=np.float64) for P in global_poses[1:]]
