// grid_lookup.h -- reading the cell-sorted target grid that the grid_* kernels of icp_kernels.hip build: which cell a
// coordinate falls in, which rows of a slab hold points, which run of the sorted target one grid row's cells hold, a
// candidate's distance, and how far a searched block of cells guarantees the nearest point.  Shared by the searches of
// icp_kernels.hip (IcpFast) and gicp_kernels.hip (the GICP neighbourhoods and correspondences), which live in different
// translation units.
#pragma once
#include "smhip_device.h"

namespace smhip {

__device__ __forceinline__ float dist2(const float4 t, float qx, float qy, float qz) {
  const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// rows y in [y0, y1] of slab z that hold points, in ascending y: f(y)
template <typename F>
__device__ __forceinline__ void for_each_occupied_row(const uint32_t* __restrict__ rb, int ny, int z, int y0, int y1, F f) {
  for (int yb = y0; yb <= y1; yb += 32) {
    const int cnt = min(32, y1 - yb + 1);
    const int ry = z * ny + yb, w = ry >> 5, sh = ry & 31;
    const unsigned long long two = (unsigned long long)rb[w] | ((unsigned long long)rb[w + 1] << 32);
    uint32_t m = (uint32_t)(two >> sh) & (cnt == 32 ? 0xffffffffu : ((1u << cnt) - 1u));
    while (m) { const int o = __ffs((int)m) - 1; m &= m - 1u; f(yb + o); }
  }
}

// occupied-cell slots [s_begin, s_end) of the cells x in [xa, xb] of one grid row
__device__ __forceinline__ void row_slots(const uint2* __restrict__ words, int rowbase, int xa, int xb,
                                          uint32_t& s_begin, uint32_t& s_end) {
  const int w0 = xa >> 5, w1 = xb >> 5;
  const uint2 a = words[rowbase + w0];
  const uint2 c = (w1 == w0) ? a : words[rowbase + w1];
  s_begin = a.y + __popc(a.x & ((1u << (xa & 31)) - 1u));
  s_end = c.y + __popc(c.x & (0xffffffffu >> (31 - (xb & 31))));
}

// distance from q to the nearest face of the cell block [X0,X1]x[Y0,Y1]x[Z0,Z1] that still has grid
// beyond it: every target point outside the block is at least that far away.  INFINITY = the block
// covers the whole grid (exhaustive).  A small fp32 slack covers points sitting on a cell face.
__device__ __forceinline__ float block_guarantee(const PairState* st, float qx, float qy, float qz,
                                                 int X0, int X1, int Y0, int Y1, int Z0, int Z1) {
  const float h = st->h;
  float g = INFINITY;
  if (X0 > 0) g = fminf(g, qx - (st->origin[0] + (float)X0 * h));
  if (X1 < st->nx - 1) g = fminf(g, (st->origin[0] + (float)(X1 + 1) * h) - qx);
  if (Y0 > 0) g = fminf(g, qy - (st->origin[1] + (float)Y0 * h));
  if (Y1 < st->ny - 1) g = fminf(g, (st->origin[1] + (float)(Y1 + 1) * h) - qy);
  if (Z0 > 0) g = fminf(g, qz - (st->origin[2] + (float)Z0 * h));
  if (Z1 < st->nz - 1) g = fminf(g, (st->origin[2] + (float)(Z1 + 1) * h) - qz);
  return g - 1.0e-3f * h;
}

__device__ __forceinline__ int cell_coord(float q, float o, float inv_h) {
  return (int)floorf(fminf(fmaxf((q - o) * inv_h, -1.0e6f), 1.0e6f));
}

}  // namespace smhip
