// smhip_submap.hip -- Submap::InsertFrame for a full submap on the device (the reference's builder/submap.cc:98-161).
//
// The reference moves every frame of a full submap into the first frame's coordinates (ApplyTransformToOutput with the frame's
// local pose, :116-119, i.e. TransformPoint per point, builder/data/cloud_types.cc:167-178), concatenates the frames (:123),
// passes the sum through a VoxelGrid of voxel_size when enable_voxel_filter is set (:144-158) and hands the result to
// CalculateNormals (:160-161).  Here the frames' raw rows go up once, ONE kernel launch covers all frames -- it reads a
// per-frame table (offset, n, pose) from device memory, writes the transformed rows and, in the same pass, the VoxelGrid key
// and row number of every point -- and the VoxelGrid of cloud_filters.hip continues from its sort.  The result is the filter
// workspace's current cloud: smhip_filter_get_output reads it, smhip_filter_output_to_source / _to_target hand it to a matcher
// slot without a download.  No atomic decides a row's place: rows are written at their own index, voxels come out in key order
// (a stable radix sort) and each voxel's double sums run in arrival order (frame order, then point order).
// smhip_submap_build_compensated_f32 is the same build with every row de-skewed by its frame's sweep motion in front of the
// transform (submap_transform_keys_comp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "smhip_context.h"
#include "motion_comp_point.h"
#include "voxel_key.h"

using namespace smhip_host;

namespace {

struct SubmapFrame {
  int32_t offset, n;        // the frame's rows are [offset, offset + n) of the concatenation
  float m[12];              // rows 0..2 of the local pose cast to float, row-major
};

// One thread per row of the concatenation.  TransformPoint: x' = ((m00 x + m01 y) + m02 z) + m03, every product and sum rounded
// to float on its own (the reference's -O2 build without -march has no fused multiply-add), as mrvm_transform does.
__global__ __launch_bounds__(256) void submap_transform_keys(const float* __restrict__ raw, int stride, const SubmapFrame* __restrict__ frames,
                                                             int n_frames, int total, float voxel_size, float4* __restrict__ pts,
                                                             float* __restrict__ fac, int32_t* __restrict__ src,
                                                             unsigned long long* __restrict__ keys, int32_t* __restrict__ idx,
                                                             int32_t* __restrict__ bad) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int lo = 0, hi = n_frames - 1;                 // the last frame whose offset is <= i (empty frames share their successor's offset)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (frames[mid].offset <= i) lo = mid; else hi = mid - 1;
  }
  const SubmapFrame f = frames[lo];
  float x, y, z, w, factor;
  if (stride == 4) {
    const float4 r = reinterpret_cast<const float4*>(raw)[i];
    x = r.x; y = r.y; z = r.z; w = r.w;
    factor = (float)((double)(i - f.offset) / (double)f.n);             // the collector's i / size (data_collector.h:202-204)
  } else {
    const float* r = raw + 5 * (size_t)i;
    x = r[0]; y = r[1]; z = r[2]; w = r[3]; factor = r[4];
  }
  float4 o;
  o.x = ((f.m[0] * x + f.m[1] * y) + f.m[2] * z) + f.m[3];
  o.y = ((f.m[4] * x + f.m[5] * y) + f.m[6] * z) + f.m[7];
  o.z = ((f.m[8] * x + f.m[9] * y) + f.m[10] * z) + f.m[11];
  o.w = w;                                                              // intensity and factor are carried unchanged
  pts[i] = o; fac[i] = factor; src[i] = i;
  if (voxel_size > 0.f) {
    unsigned long long k;
    if (!voxel_key(o, voxel_size, k)) *bad = 1;                         // (every writer stores the same value)
    keys[i] = k; idx[i] = i;
  }
}

// The compensated build: the same pass with MotionCompensation (motion_comp_point.h) of the row under the frame's own sweep motion
// in front of the local TransformPoint -- the de-skewed coordinates are rounded to float once, as a stored de-skewed cloud would hold
// them, and go nowhere but into the transform.  A kernel of its own, so that submap_transform_keys stays the code it is; the frame
// table carries the frame's MotionCompArgs next to m[12].  A factor outside [0, 1] or NaN raises *bad_factor by a plain store and
// the row is transformed as it is.  Key, src, fac and *bad are submap_transform_keys'.
struct SubmapFrameComp {
  int32_t offset, n;
  float m[12];
  MotionCompArgs motion;
};

__global__ __launch_bounds__(256) void submap_transform_keys_comp(const float* __restrict__ raw, int stride,
                                                                  const SubmapFrameComp* __restrict__ frames, int n_frames, int total,
                                                                  float voxel_size, float4* __restrict__ pts, float* __restrict__ fac,
                                                                  int32_t* __restrict__ src, unsigned long long* __restrict__ keys,
                                                                  int32_t* __restrict__ idx, int32_t* __restrict__ bad,
                                                                  int32_t* __restrict__ bad_factor) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int lo = 0, hi = n_frames - 1;                 // the last frame whose offset is <= i (empty frames share their successor's offset)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (frames[mid].offset <= i) lo = mid; else hi = mid - 1;
  }
  const SubmapFrameComp& f = frames[lo];
  const int offset = f.offset;
  float x, y, z, w, factor;
  if (stride == 4) {
    const float4 r = reinterpret_cast<const float4*>(raw)[i];
    x = r.x; y = r.y; z = r.z; w = r.w;
    factor = (float)((double)(i - offset) / (double)f.n);               // the collector's i / size (data_collector.h:202-204)
  } else {
    const float* r = raw + 5 * (size_t)i;
    x = r[0]; y = r[1]; z = r[2]; w = r[3]; factor = r[4];
  }
  if (motion_comp_factor_ok(factor)) {
    const float3 q = motion_comp_point(f.motion, x, y, z, factor);
    x = q.x; y = q.y; z = q.z;
  } else {
    *bad_factor = 1;                                                     // (every writer stores the same value)
  }
  float4 o;
  o.x = ((f.m[0] * x + f.m[1] * y) + f.m[2] * z) + f.m[3];
  o.y = ((f.m[4] * x + f.m[5] * y) + f.m[6] * z) + f.m[7];
  o.z = ((f.m[8] * x + f.m[9] * y) + f.m[10] * z) + f.m[11];
  o.w = w;
  pts[i] = o; fac[i] = factor; src[i] = i;
  if (voxel_size > 0.f) {
    unsigned long long k;
    if (!voxel_key(o, voxel_size, k)) *bad = 1;
    keys[i] = k; idx[i] = i;
  }
}

// Both builds.  motions == nullptr: the plain one; otherwise 16 doubles per frame (column-major), the sensor's motion during that
// frame's sweep, and the compensated kernel.
smhip_status submap_build(smhip_handle h, int n_frames, const float* const* rows, int stride_floats, const int* n, const double* local_poses,
                          const double* motions, float voxel_size, int* n_out) {
  if (n_frames < 1 || !rows || !n || !local_poses || (stride_floats != 4 && stride_floats != 5)) {
    h->err = "bad arguments (n_frames >= 1, frame tables, stride 4 = x y z intensity or 5 = InnerPointType)";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  // 0 = no voxel filter; otherwise VoxelGrid::ConfigsValid(), filter_voxel_grid.cc:36
  if (!std::isfinite(voxel_size) || voxel_size < 0.f || (voxel_size > 0.f && !(voxel_size > 1.e-6))) {
    h->err = "voxel_size must be 0 (no voxel filter) or a finite number above 1e-6";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  long long total = 0;
  for (int k = 0; k < n_frames; ++k) {
    if (n[k] < 0 || (n[k] > 0 && !rows[k])) { h->err = "frame " + std::to_string(k) + ": negative size or null rows"; return SMHIP_ERR_INVALID_ARGUMENT; }
    for (int q = 0; q < 16; ++q) {
      if (!std::isfinite(local_poses[16 * (size_t)k + q])) { h->err = "frame " + std::to_string(k) + ": pose is not finite"; return SMHIP_ERR_INVALID_ARGUMENT; }
      if (motions && !std::isfinite(motions[16 * (size_t)k + q])) { h->err = "frame " + std::to_string(k) + ": motion is not finite"; return SMHIP_ERR_INVALID_ARGUMENT; }
    }
    total += n[k];
  }
  if (total == 0) { h->err = "every frame is empty"; return SMHIP_ERR_INVALID_ARGUMENT; }
  const int cap = std::max(h->dev.ns_cap, h->dev.nt_cap);
  if (total > cap) { h->err = "the frames together are larger than the handle's capacity"; return SMHIP_ERR_CAPACITY; }
  const int N = (int)total;
  HIPCHK(h, hipSetDevice(h->device));
  smhip_status s = filter_ensure(h);
  if (s) return s;
  if (!h->submap_raw) { s = dev_alloc(h, &h->submap_raw, 5 * (size_t)cap); if (s) return s; }
  if (n_frames > h->submap_frames_cap) {         // (an outgrown table stays with the handle's allocations until smhip_destroy)
    const int want = std::max(64, std::max(n_frames, 2 * h->submap_frames_cap));
    SubmapFrameComp* t = nullptr;                // room for the larger of the two tables' entries
    s = dev_alloc(h, &t, (size_t)want);
    if (s) return s;
    h->submap_frames = t; h->submap_frames_cap = want;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // the rows travel as they are, frame after frame, through the page-locked staging array (2 float4 per point of capacity)
  std::vector<SubmapFrame> table(motions ? 0 : (size_t)n_frames);
  std::vector<SubmapFrameComp> table_comp(motions ? (size_t)n_frames : 0);
  float* stage = reinterpret_cast<float*>(h->stage);
  int offset = 0;
  for (int k = 0; k < n_frames; ++k) {
    float* m = motions ? table_comp[k].m : table[k].m;
    if (motions) { table_comp[k].offset = offset; table_comp[k].n = n[k]; table_comp[k].motion = motion_comp_args(motions + 16 * (size_t)k); }
    else { table[k].offset = offset; table[k].n = n[k]; }
    const double* P = local_poses + 16 * (size_t)k;                      // column-major; cast to float as TransformPoint does
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m[4 * r + c] = (float)P[4 * c + r];
    if (n[k] > 0) std::memcpy(stage + (size_t)stride_floats * offset, rows[k], sizeof(float) * (size_t)stride_floats * n[k]);
    offset += n[k];
  }
  HIPCHK(h, hipMemcpyAsync(h->submap_raw, stage, sizeof(float) * (size_t)stride_floats * N, hipMemcpyHostToDevice, h->stream));
  if (motions) HIPCHK(h, hipMemcpyAsync(h->submap_frames, table_comp.data(), sizeof(SubmapFrameComp) * (size_t)n_frames, hipMemcpyHostToDevice, h->stream));
  else HIPCHK(h, hipMemcpyAsync(h->submap_frames, table.data(), sizeof(SubmapFrame) * (size_t)n_frames, hipMemcpyHostToDevice, h->stream));
  const FilterBuild b = filt_build_begin(h->filt, h->stream);
  if (!b.pts) { h->err = "filter workspace not available"; return SMHIP_ERR_HIP; }
  bool bad_factor = false;
  if (motions) {
    int32_t* flag = filt_motion_flag_begin(h->filt, h->stream);
    if (!flag) { h->err = "filter workspace not available"; return SMHIP_ERR_HIP; }
    hipLaunchKernelGGL(submap_transform_keys_comp, dim3((N + 255) / 256), dim3(256), 0, h->stream, h->submap_raw, stride_floats,
                       static_cast<const SubmapFrameComp*>(h->submap_frames), n_frames, N, voxel_size, b.pts, b.fac, b.src, b.keys, b.idx, b.bad, flag);
    HIPCHK(h, hipGetLastError());
    // the factor flag is read before the commit (one synchronise more than the plain build): with a bad factor the rows are
    // committed as they were written, with no VoxelGrid, so that the unfiltered concatenation is what stays resident
    HIPCHK(h, filt_motion_flag_end(h->filt, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    bad_factor = filt_motion_bad_factor(h->filt);
  } else {
    hipLaunchKernelGGL(submap_transform_keys, dim3((N + 255) / 256), dim3(256), 0, h->stream, h->submap_raw, stride_floats,
                       static_cast<const SubmapFrame*>(h->submap_frames), n_frames, N, voxel_size, b.pts, b.fac, b.src, b.keys, b.idx, b.bad);
    HIPCHK(h, hipGetLastError());
  }
  const hipError_t e = filt_build_commit(h->filt, h->stream, N, voxel_size > 0.f && !bad_factor, n_out);
  if (e != hipSuccess) {
    h->err = e == hipErrorInvalidValue ? "submap build: a voxel index lies beyond +-2^20 (the unfiltered rows stay resident)"
                                       : std::string("submap build: ") + hipGetErrorString(e);
    return e == hipErrorInvalidValue ? SMHIP_ERR_INVALID_ARGUMENT : SMHIP_ERR_HIP;
  }
  if (bad_factor) {
    h->err = "submap build: a row's factor is outside [0, 1] or NaN (CHECK(factor >= 0. && factor <= 1.), common/math.h:202; the unfiltered "
             "rows stay resident)";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  return SMHIP_OK;
}

}  // namespace

extern "C" {

smhip_status smhip_submap_build_f32(smhip_handle h, int n_frames, const float* const* rows, int stride_floats, const int* n,
                                    const double* local_poses, float voxel_size, int* n_out) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  return submap_build(h, n_frames, rows, stride_floats, n, local_poses, nullptr, voxel_size, n_out);
}

smhip_status smhip_submap_build_compensated_f32(smhip_handle h, int n_frames, const float* const* rows, int stride_floats, const int* n,
                                                const double* local_poses, const double* motions, float voxel_size, int* n_out) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  if (!motions) { h->err = "null motions (one 4x4 per frame)"; return SMHIP_ERR_INVALID_ARGUMENT; }
  return submap_build(h, n_frames, rows, stride_floats, n, local_poses, motions, voxel_size, n_out);
}

// the resident cloud goes through the device CalculateNormals into the target of `slot` (submap.cc:160-161)
smhip_status smhip_filter_output_to_target(smhip_handle h, int slot, int* n_out) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!h->filt || filt_count(h->filt) <= 0) { h->err = "no filtered or built cloud is resident"; return SMHIP_ERR_NOT_READY; }
  HIPCHK(h, hipSetDevice(h->device));
  s = prep_ensure(h);
  if (s) return s;
  return prep_run(h, filt_points(h->filt), filt_count(h->filt), slot, n_out);
}

}  // extern "C"
