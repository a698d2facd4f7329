// voxel_key.h -- the packed VoxelGrid key (filter_voxel_grid.cc:51-53) shared by the kernels that write it: filt_voxel_keys in
// cloud_filters.hip and submap_transform_keys in smhip_submap.hip.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace smhip {

constexpr long kVoxBias = 1l << 20;            // 21 bits per axis
// false (and key = all ones) when an index leaves +-2^20; an infinite coordinate does, a NaN is not told apart here
__device__ __forceinline__ bool voxel_key(const float4 p, float size, unsigned long long& key) {
  const long ix = lroundf(p.x / size), iy = lroundf(p.y / size), iz = lroundf(p.z / size);   // filter_voxel_grid.cc:51-53
  const long a = ix + kVoxBias, b = iy + kVoxBias, c = iz + kVoxBias;
  const bool ok = a >= 0 && a < 2 * kVoxBias && b >= 0 && b < 2 * kVoxBias && c >= 0 && c < 2 * kVoxBias;
  key = ok ? (((unsigned long long)a << 42) | ((unsigned long long)b << 21) | (unsigned long long)c) : ~0ull;
  return ok;
}

}  // namespace smhip
