// cloud_filters.hip -- the front end's point-cloud pre-filters on the device.
//
// Reference: /root/reference/pre_processors/
//   filter_range.cc:46-91          Range               keep min_range <= |p| <= max_range (float norm)
//   filter_axis_range.cc:45-103    AxisRange           keep min <= p[axis] <= max
//   filter_bounding_box.cc:53-83   BoundingBoxRemoval  DROP the points inside [min, max] (common/bounding_box.cc:117-121)
//   filter_random_sample.cc:41-85  RandomSampler       keep a point when a uniform draw <= sampling_rate
//   filter_voxel_grid.cc:38-80     VoxelGrid           one average point (double sums) per lround(p / size) voxel
//   filter_ground_removal.cc        GroundRemoval       drop small voxels and flat low ones    } kernels in ground_filters.hip;
//   filter_ground_removal2.cc       GroundRemoval2      drop points near fitted ground lines   } what is and is not pinned:
//   filter_range_image.cc           RangeImage          keep the first point of every pixel    } DESIGN.md §6, "Pre-filters"
//   filter_statistic_removal.cc     StatisticRemoval    drop rows far from their k nearest neighbours (kernels in
//                                                       statistic_removal.hip; the definition: DESIGN.md §6, "StatisticRemoval")
//   filter_factory.cc:83-106       Factory::Filter     the filters of <filters> applied in order
//   builder/map_builder.cc:232-257  MotionCompensation  the front end's de-skew of the filtered cloud (kernel in motion_comp.hip)
// They run on every scan right before the registrator (builder/data/data_collector.h, config/lidar_only_kitti.xml:18-41).
// All but VoxelGrid are order-preserving compactions: flag -> exclusive scan (rocPRIM building block) -> scatter;
// consecutive predicate filters share one pass.  VoxelGrid is a stable radix sort on the packed voxel index and one
// thread per voxel summing its points in arrival order in double, so each output point carries the reference's bits
// (the reference emits voxels in unordered_map order, i.e. unspecified; here they come out sorted by voxel index).
// The three ground / image filters end in the same flag -> scan -> scatter, so their output keeps the input order (GroundRemoval
// emits voxel by voxel in the reference, in std::map order of the voxel index; GroundRemoval2 and RangeImage keep input order).
// Every chain runs on smhip_filter_desc_ex; smhip_filter_chain_f32 widens its descriptors first.
#include <cstring>
#include <string>
#include <string.h>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/smhip.h"
#include "cloud_filters.h"
#include "motion_comp_point.h"
#include "voxel_key.h"

namespace smhip {

namespace {

constexpr int kMaxFused = 8;
struct Pred { int32_t type; int32_t axis; float p[6]; };
struct PredGroup { int32_t n; Pred f[kMaxFused]; };

// filter_range.cc:60-66 without fused multiply-adds (the reference's float expression, operation by operation)
__device__ __forceinline__ bool keep_point(const Pred& f, const float4 p) {
  switch (f.type) {
    case SMHIP_FILTER_RANGE: {
      const float r = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y)), __fmul_rn(p.z, p.z)));
      return r >= f.p[0] && r <= f.p[1];
    }
    case SMHIP_FILTER_AXIS_RANGE: {
      const float v = f.axis == 0 ? p.x : (f.axis == 1 ? p.y : p.z);
      return !(v < f.p[0] || v > f.p[1]);                                  // filter_axis_range.cc:68-86
    }
    case SMHIP_FILTER_BOUNDING_BOX_REMOVAL: {
      const double x = p.x, y = p.y, z = p.z;                              // Eigen::Vector3d(point.x, ...), :72
      const bool inside = (x >= (double)f.p[0] && x <= (double)f.p[3]) && (y >= (double)f.p[1] && y <= (double)f.p[4]) &&
                          (z >= (double)f.p[2] && z <= (double)f.p[5]);
      return !inside;
    }
  }
  return true;
}

__global__ void filt_flags(const float4* pts, int n, PredGroup g, int32_t* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  bool k = true;
  for (int q = 0; q < g.n; ++q) k = k && keep_point(g.f[q], p);
  flag[i] = k ? 1 : 0;
}

// counter-based uniform in [0, 1): the reference seeds a mt19937 from std::random_device on every call
// (filter_random_sample.cc:57-59), so no particular stream can be reproduced; what is kept is the law:
// one uniform double per input point of THIS filter, kept when u <= sampling_rate.
__device__ __forceinline__ double sampler_uniform(uint32_t seed, uint32_t i) {
  unsigned long long z = ((unsigned long long)seed << 32 | i) + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
__global__ void filt_sample_flags(int n, uint32_t seed, float rate, int32_t* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flag[i] = sampler_uniform(seed, (uint32_t)i) <= (double)rate ? 1 : 0;   // distr(eng) <= sampling_rate_, :68
}

__global__ void filt_scatter(const float4* pts, const float* fac, const int32_t* src, int n, const int32_t* flag, const int32_t* pos,
                             float4* out_pts, float* out_fac, int32_t* out_src, int32_t* count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flag[i]) {
    const int o = pos[i];
    out_pts[o] = pts[i]; out_fac[o] = fac[i]; out_src[o] = src[i];
  }
  if (i == n - 1) count[0] = pos[i] + flag[i];
}

// ---- VoxelGrid ---------------------------------------------------------------------------------
__global__ void filt_voxel_keys(const float4* pts, int n, float size, unsigned long long* keys, int32_t* idx, int32_t* bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long k;
  if (!voxel_key(pts[i], size, k)) atomicAdd(bad, 1);
  keys[i] = k; idx[i] = i;
}
__global__ void filt_voxel_heads(const unsigned long long* keys, int n, int32_t* head) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  head[s] = (s == 0 || keys[s] != keys[s - 1]) ? 1 : 0;
}
__global__ void filt_voxel_starts(const int32_t* head, const int32_t* incl, int n, int32_t* start, int32_t* count) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  if (head[s]) start[incl[s] - 1] = s;
  if (s == n - 1) count[0] = incl[s];
}
__global__ void filt_voxel_average(const float4* pts, const int32_t* idx, const int32_t* start, const int32_t* count, int n,
                                   float4* out_pts, float* out_fac, int32_t* out_src) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const int V = count[0];
  if (v >= V) return;
  const int a = start[v], b = (v + 1 < V) ? start[v + 1] : n;
  double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
  for (int s = a; s < b; ++s) { const float4 p = pts[idx[s]]; s0 += p.x; s1 += p.y; s2 += p.z; s3 += p.w; }   // :61-66
  const int size = b - a;
  out_pts[v] = make_float4((float)(s0 / size), (float)(s1 / size), (float)(s2 / size), (float)(s3 / size));   // :68-74
  out_fac[v] = 0.f;                              // InnerPointType result: factor keeps its default
  out_src[v] = -1;
}

#include "ground_filters.hip"
#include "motion_comp.hip"
#include "statistic_removal.hip"

__global__ void filt_init(const float4* in, int n, int stride5, const float* fac_in, float4* pts, float* fac, int32_t* src) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pts[i] = in[i];
  // stride 5 rows carry their factor; KITTI rows get the collector's i / size (data_collector.h:202-204)
  fac[i] = stride5 ? fac_in[i] : (float)((double)i / (double)n);
  src[i] = i;
}

}  // namespace

struct FilterWorkspace {
  int cap = 0;
  float4* pts[2] = {nullptr, nullptr};
  float* fac[2] = {nullptr, nullptr};
  int32_t* src[2] = {nullptr, nullptr};
  int32_t *flag = nullptr, *pos = nullptr, *idx[2] = {nullptr, nullptr}, *start = nullptr, *counts = nullptr;
  unsigned long long* keys[2] = {nullptr, nullptr};
  float* fac_in = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  int32_t* host_pinned = nullptr;
  int cur = 0;              // which of pts[2] holds the current cloud
  int n = 0;
  bool has_index = true;    // false once a VoxelGrid has run
  // the ground / image filters' tables: allocated on first use, grown when a larger grid or image comes
  float *gd = nullptr, *gz = nullptr, *runmin = nullptr;   // cap floats each (GroundRemoval2, per sorted point)
  int32_t *vmin = nullptr, *vmax = nullptr;                // cap each (GroundRemoval, per voxel)
  int grid_cap = 0;                                        // GroundRemoval2: S * B grids and line slots
  int32_t *gend = nullptr, *gfirst = nullptr, *nlines = nullptr;
  float4* lines = nullptr;
  int seg_cap = 0;
  int pix_cap = 0;                                         // RangeImage: V * H pixels
  int32_t* pix = nullptr;
  // StatisticRemoval: allocated on first use for the workspace's capacity
  float4* sr_pts = nullptr;                                // the finite rows sorted along the search axis
  float* sr_dist = nullptr;                                // distance[] of the last StatisticRemoval, in its input row order
  double *sr_csum = nullptr, *sr_csq = nullptr, *sr_stat = nullptr;   // sums per 64 rows; sum, sq_sum, V, threshold
  uint32_t* sr_meta = nullptr;                             // bounding box of the finite rows and their number
  int sr_rows = -1;                                        // rows that filter saw in the last chain; -1 none ran, -2 it passed the cloud through
  std::string note;                                        // a warning the last chain leaves for the handle's last-error text
};

FilterWorkspace* filt_create(int max_points) {
  FilterWorkspace* w = new FilterWorkspace();
  w->cap = max_points;
  const size_t N = (size_t)max_points;
  bool ok = true;
  auto A = [&](void** p, size_t bytes) { if (ok && hipMalloc(p, bytes) != hipSuccess) ok = false; };
  for (int k = 0; k < 2; ++k) {
    A((void**)&w->pts[k], N * sizeof(float4)); A((void**)&w->fac[k], N * 4); A((void**)&w->src[k], N * 4);
    A((void**)&w->idx[k], N * 4); A((void**)&w->keys[k], N * 8);
  }
  A((void**)&w->flag, N * 4); A((void**)&w->pos, N * 4); A((void**)&w->start, N * 4); A((void**)&w->counts, 16 * 4);
  A((void**)&w->fac_in, N * 4);
  if (ok) {
    size_t b1 = 0, b2 = 0;
    (void)rocprim::radix_sort_pairs(nullptr, b1, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                    (const int32_t*)nullptr, (int32_t*)nullptr, (unsigned)max_points, 0, 64, (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, b2, (const int32_t*)nullptr, (int32_t*)nullptr, 0, N, rocprim::plus<int32_t>(), (hipStream_t)0);
    w->tmp_bytes = std::max(b1, b2) + 256;
    A(&w->tmp, w->tmp_bytes);
  }
  if (ok && hipHostMalloc((void**)&w->host_pinned, 64) != hipSuccess) ok = false;
  if (!ok) { filt_destroy(w); return nullptr; }
  return w;
}

void filt_destroy(FilterWorkspace* w) {
  if (!w) return;
  for (int k = 0; k < 2; ++k) {
    (void)hipFree(w->pts[k]); (void)hipFree(w->fac[k]); (void)hipFree(w->src[k]); (void)hipFree(w->idx[k]); (void)hipFree(w->keys[k]);
  }
  (void)hipFree(w->flag); (void)hipFree(w->pos); (void)hipFree(w->start); (void)hipFree(w->counts); (void)hipFree(w->fac_in);
  (void)hipFree(w->tmp);
  (void)hipFree(w->gd); (void)hipFree(w->gz); (void)hipFree(w->runmin); (void)hipFree(w->vmin); (void)hipFree(w->vmax);
  (void)hipFree(w->gend); (void)hipFree(w->gfirst); (void)hipFree(w->nlines); (void)hipFree(w->lines); (void)hipFree(w->pix);
  (void)hipFree(w->sr_pts); (void)hipFree(w->sr_dist); (void)hipFree(w->sr_csum); (void)hipFree(w->sr_csq); (void)hipFree(w->sr_stat);
  (void)hipFree(w->sr_meta);
  if (w->host_pinned) (void)hipHostFree(w->host_pinned);
  delete w;
}

#define FCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return e_; } while (0)

hipError_t filt_set_input(FilterWorkspace* w, hipStream_t st, const float4* staged_dev, const float* factor_host_or_null, int n) {
  if (!w || n < 0 || n > w->cap) return hipErrorInvalidValue;
  w->cur = 0; w->n = n; w->has_index = true;
  if (n == 0) return hipSuccess;
  if (factor_host_or_null) FCHK(hipMemcpyAsync(w->fac_in, factor_host_or_null, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(filt_init, dim3((n + 255) / 256), dim3(256), 0, st, staged_dev, n, factor_host_or_null ? 1 : 0, w->fac_in,
                     w->pts[0], w->fac[0], w->src[0]);
  return hipGetLastError();
}

static hipError_t compact(FilterWorkspace* w, hipStream_t st) {      // flags are in w->flag
  const int n = w->n, c = w->cur, o = 1 - c;
  size_t bytes = w->tmp_bytes;
  FCHK(rocprim::exclusive_scan(w->tmp, bytes, w->flag, w->pos, 0, (size_t)n, rocprim::plus<int32_t>(), st));
  hipLaunchKernelGGL(filt_scatter, dim3((n + 255) / 256), dim3(256), 0, st, w->pts[c], w->fac[c], w->src[c], n, w->flag, w->pos,
                     w->pts[o], w->fac[o], w->src[o], w->counts);
  FCHK(hipMemcpyAsync(w->host_pinned, w->counts, 4, hipMemcpyDeviceToHost, st));
  FCHK(hipStreamSynchronize(st));
  w->n = w->host_pinned[0];
  w->cur = o;
  return hipSuccess;
}

static hipError_t grow(void** p, size_t bytes) {
  (void)hipFree(*p);
  *p = nullptr;
  return hipMalloc(p, bytes);
}

// the per-point tables of the ground filters and a temporary buffer large enough for the segmented scan
static hipError_t ensure_ground(FilterWorkspace* w) {
  if (w->gd) return hipSuccess;
  const size_t N = (size_t)std::max(w->cap, 1);
  FCHK(hipMalloc((void**)&w->gd, N * 4)); FCHK(hipMalloc((void**)&w->gz, N * 4)); FCHK(hipMalloc((void**)&w->runmin, N * 4));
  FCHK(hipMalloc((void**)&w->vmin, N * 4)); FCHK(hipMalloc((void**)&w->vmax, N * 4));
  size_t b = 0;
  FCHK(rocprim::inclusive_scan_by_key(nullptr, b, (const unsigned long long*)nullptr, (const float*)nullptr, (float*)nullptr, N,
                                      rocprim::minimum<float>(), rocprim::equal_to<unsigned long long>(), (hipStream_t)0));
  if (b + 256 > w->tmp_bytes) {
    FCHK(grow(&w->tmp, b + 256));
    w->tmp_bytes = b + 256;
  }
  return hipSuccess;
}

static int key_bits(unsigned long long max_key) { int b = 1; while (b < 64 && (max_key >> b) != 0) ++b; return b; }

// GroundRemoval2 on the current cloud: bin -> stable sort by grid -> segmented running minimum -> line fits -> cluster -> compact
static hipError_t run_ground_removal2(FilterWorkspace* w, hipStream_t st, const smhip_filter_desc_ex& f) {
  const int n = w->n, gp = (n + 255) / 256, c = w->cur;
  const int B = f.i[0], S = f.i[1], G = B * S;
  FCHK(ensure_ground(w));
  if (G > w->grid_cap) {
    FCHK(grow((void**)&w->gend, (size_t)G * 4)); FCHK(grow((void**)&w->gfirst, (size_t)G * 4));
    FCHK(grow((void**)&w->lines, (size_t)G * sizeof(float4)));
    w->grid_cap = G;
  }
  if (S > w->seg_cap) { FCHK(grow((void**)&w->nlines, (size_t)S * 4)); w->seg_cap = S; }
  Gr2Args a{};
  a.two_pi = (float)(M_PI * 2);                                          // const float double_pi = M_PI * 2, :146
  a.delta_alpha = a.two_pi / (float)S;
  a.delta_bin = (f.p[0] - f.p[1]) / (float)B;
  a.r_min = f.p[1];
  a.start_h = f.p[2]; a.long_thr = f.p[3]; a.long_h = f.p[4]; a.start_max = f.p[5]; a.max_err = f.p[6]; a.max_slope = f.p[7];
  a.max_dist = f.p[9];
  a.B = B; a.S = S; a.G = G;
  a.search_step = gr2_search_step(f.p[10], S);
  hipLaunchKernelGGL(gr2_bin, dim3(gp), dim3(256), 0, st, w->pts[c], n, a, w->keys[0], w->idx[0]);
  size_t bytes = w->tmp_bytes;
  FCHK(rocprim::radix_sort_pairs(w->tmp, bytes, w->keys[0], w->keys[1], w->idx[0], w->idx[1], (unsigned)n, 0, key_bits((unsigned long long)G), st));
  hipLaunchKernelGGL(gr2_gather, dim3(gp), dim3(256), 0, st, w->pts[c], w->keys[1], w->idx[1], n, G, w->gd, w->gz, w->gend);
  bytes = w->tmp_bytes;
  FCHK(rocprim::inclusive_scan_by_key(w->tmp, bytes, w->keys[1], w->gz, w->runmin, (size_t)n, rocprim::minimum<float>(),
                                      rocprim::equal_to<unsigned long long>(), st));
  FCHK(hipMemsetD32Async((hipDeviceptr_t)w->gfirst, INT_MAX, (size_t)G, st));
  hipLaunchKernelGGL(gr2_mark, dim3(gp), dim3(256), 0, st, w->keys[1], w->gz, w->runmin, w->gend, n, G, w->start, w->gfirst);
  hipLaunchKernelGGL(gr2_fit_lines, dim3(S), dim3(64), sizeof(float2) * (size_t)B, st, w->gd, w->gz, w->gfirst, a, w->lines, w->nlines);
  hipLaunchKernelGGL(gr2_cluster, dim3(gp), dim3(256), 0, st, w->keys[1], w->idx[1], w->gd, w->gz, w->start, n, a, w->lines, w->nlines,
                     w->flag);
  return compact(w, st);
}

// GroundRemoval on the current cloud: truncated voxel keys -> radix sort -> per-voxel size and z range -> flags -> compact
static hipError_t run_ground_removal(FilterWorkspace* w, hipStream_t st, const smhip_filter_desc_ex& f) {
  const int n = w->n, gp = (n + 255) / 256, c = w->cur;
  FCHK(ensure_ground(w));
  FCHK(hipMemsetAsync(w->counts + 1, 0, 4, st));
  hipLaunchKernelGGL(gr_keys, dim3(gp), dim3(256), 0, st, w->pts[c], n, f.p[0], w->keys[0], w->idx[0], w->counts + 1);
  size_t bytes = w->tmp_bytes;
  FCHK(rocprim::radix_sort_pairs(w->tmp, bytes, w->keys[0], w->keys[1], w->idx[0], w->idx[1], (unsigned)n, 0, 64, st));
  hipLaunchKernelGGL(filt_voxel_heads, dim3(gp), dim3(256), 0, st, w->keys[1], n, w->flag);
  bytes = w->tmp_bytes;
  FCHK(rocprim::inclusive_scan(w->tmp, bytes, w->flag, w->pos, (size_t)n, rocprim::plus<int32_t>(), st));
  hipLaunchKernelGGL(filt_voxel_starts, dim3(gp), dim3(256), 0, st, w->flag, w->pos, n, w->start, w->counts);
  FCHK(hipMemsetD32Async((hipDeviceptr_t)w->vmin, INT_MAX, (size_t)n, st));
  FCHK(hipMemsetD32Async((hipDeviceptr_t)w->vmax, INT_MIN, (size_t)n, st));
  hipLaunchKernelGGL(gr_minmax, dim3(gp), dim3(256), 0, st, w->pts[c], w->keys[1], w->idx[1], w->pos, n, w->vmin, w->vmax);
  hipLaunchKernelGGL(gr_flags, dim3(gp), dim3(256), 0, st, w->keys[1], w->idx[1], w->pos, w->start, w->counts, n, f.p[1], f.i[0],
                     w->vmin, w->vmax, w->flag);
  FCHK(hipMemcpyAsync(w->host_pinned + 2, w->counts + 1, 4, hipMemcpyDeviceToHost, st));
  FCHK(hipStreamSynchronize(st));
  if (w->host_pinned[2] != 0) return hipErrorInvalidValue;               // a voxel index beyond +-2^20
  return compact(w, st);
}

// RangeImage::Filter on the current cloud: pixel per row, atomicMin of the row index per pixel, keep the winners
static hipError_t run_range_image(FilterWorkspace* w, hipStream_t st, const smhip_filter_desc_ex& f) {
  const int n = w->n, gp = (n + 255) / 256, c = w->cur;
  const int V = f.i[0], H = f.i[1];
  if (V * H > w->pix_cap) { FCHK(grow((void**)&w->pix, (size_t)V * H * 4)); w->pix_cap = V * H; }
  RiArgs a{};
  a.ox = f.p[2]; a.oy = f.p[3]; a.oz = f.p[4];
  a.hres = (float)(M_PI * 2 / (double)(float)H);                        // :84-85
  a.vres = (float)((double)((f.p[0] - f.p[1]) / (float)V / 180.f) * M_PI);   // :86-88
  a.btm_rad = (double)(f.p[1] / 180.f) * M_PI;                          // :105
  a.V = V; a.H = H;
  FCHK(hipMemsetD32Async((hipDeviceptr_t)w->pix, INT_MAX, (size_t)V * H, st));
  hipLaunchKernelGGL(ri_pixel, dim3(gp), dim3(256), 0, st, w->pts[c], n, a, w->idx[0], w->pix);
  hipLaunchKernelGGL(ri_flags, dim3(gp), dim3(256), 0, st, w->idx[0], w->pix, n, w->flag);
  return compact(w, st);
}

// VoxelGrid from the keys on: keys[0] / idx[0] hold the current cloud's packed voxel keys and row numbers, counts[1] is non-zero
// when a voxel index left +-2^20.  Stable radix sort -> voxel heads -> starts -> one thread per voxel averaging in arrival order.
static hipError_t voxel_tail(FilterWorkspace* w, hipStream_t st) {
  const int n = w->n, gp = (n + 255) / 256, c = w->cur, o = 1 - c;
  size_t bytes = w->tmp_bytes;
  FCHK(rocprim::radix_sort_pairs(w->tmp, bytes, w->keys[0], w->keys[1], w->idx[0], w->idx[1], (unsigned)n, 0, 64, st));
  hipLaunchKernelGGL(filt_voxel_heads, dim3(gp), dim3(256), 0, st, w->keys[1], n, w->flag);
  bytes = w->tmp_bytes;
  FCHK(rocprim::inclusive_scan(w->tmp, bytes, w->flag, w->pos, (size_t)n, rocprim::plus<int32_t>(), st));
  hipLaunchKernelGGL(filt_voxel_starts, dim3(gp), dim3(256), 0, st, w->flag, w->pos, n, w->start, w->counts);
  hipLaunchKernelGGL(filt_voxel_average, dim3(gp), dim3(256), 0, st, w->pts[c], w->idx[1], w->start, w->counts, n,
                     w->pts[o], w->fac[o], w->src[o]);
  FCHK(hipMemcpyAsync(w->host_pinned, w->counts, 8, hipMemcpyDeviceToHost, st));
  FCHK(hipStreamSynchronize(st));
  if (w->host_pinned[1] != 0) return hipErrorInvalidValue;             // a voxel index beyond +-2^20
  w->n = w->host_pinned[0];
  w->cur = o;
  w->has_index = false;
  return hipSuccess;
}

static hipError_t ensure_statistic(FilterWorkspace* w) {
  if (w->sr_meta) return hipSuccess;
  const size_t N = (size_t)std::max(w->cap, 1), C = N / 64 + 1;
  FCHK(hipMalloc((void**)&w->sr_pts, N * sizeof(float4))); FCHK(hipMalloc((void**)&w->sr_dist, N * 4));
  FCHK(hipMalloc((void**)&w->sr_csum, C * 8)); FCHK(hipMalloc((void**)&w->sr_csq, C * 8)); FCHK(hipMalloc((void**)&w->sr_stat, 4 * 8));
  return hipMalloc((void**)&w->sr_meta, 8 * 4);
}

static double sr_unordered(uint32_t o) {                 // the float behind an sr_ordered word
  const uint32_t u = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
  float f;
  std::memcpy(&f, &u, 4);
  return (double)f;
}

// StatisticRemoval on the current cloud: bounding box and V -> sort along the longest side -> k-NN mean distances -> the two
// sums and the threshold -> flags -> compact.  V <= k keeps every row and leaves a warning.
static hipError_t run_statistic_removal(FilterWorkspace* w, hipStream_t st, const smhip_filter_desc_ex& f) {
  const int n = w->n, gp = (n + 255) / 256, c = w->cur, k = f.i[0];
  FCHK(ensure_statistic(w));
  FCHK(hipMemsetD32Async((hipDeviceptr_t)w->sr_meta, -1, 3, st));
  FCHK(hipMemsetAsync(w->sr_meta + 3, 0, 4 * 4, st));
  hipLaunchKernelGGL(sr_extent, dim3(std::min(gp, 64)), dim3(256), 0, st, w->pts[c], n, w->sr_meta);
  FCHK(hipMemcpyAsync(w->host_pinned + 4, w->sr_meta, 7 * 4, hipMemcpyDeviceToHost, st));
  FCHK(hipStreamSynchronize(st));
  const uint32_t* meta = reinterpret_cast<const uint32_t*>(w->host_pinned + 4);
  const int V = (int)meta[6];
  if (V <= k) {
    w->sr_rows = -2;
    w->note = "warning: StatisticRemoval kept every row: " + std::to_string(V) + " finite row(s) for point_num_meank = " + std::to_string(k);
    return hipSuccess;
  }
  double ext[3];
  for (int a = 0; a < 3; ++a) ext[a] = sr_unordered(meta[3 + a]) - sr_unordered(meta[a]);
  const int axis = (ext[0] >= ext[1] && ext[0] >= ext[2]) ? 0 : (ext[1] >= ext[2] ? 1 : 2);
  hipLaunchKernelGGL(sr_keys, dim3(gp), dim3(256), 0, st, w->pts[c], n, axis, w->keys[0], w->idx[0]);
  size_t bytes = w->tmp_bytes;
  FCHK(rocprim::radix_sort_pairs(w->tmp, bytes, w->keys[0], w->keys[1], w->idx[0], w->idx[1], (unsigned)n, 0, 32, st));
  hipLaunchKernelGGL(sr_gather, dim3((V + 255) / 256), dim3(256), 0, st, w->pts[c], w->idx[1], V, axis, w->sr_pts);
  const dim3 gk((n + kSrThreads - 1) / kSrThreads), bk(kSrThreads);
  if (k <= 16) hipLaunchKernelGGL(sr_knn<16>, gk, bk, 0, st, w->sr_pts, w->idx[1], V, n, k, w->sr_dist);
  else if (k <= 32) hipLaunchKernelGGL(sr_knn<32>, gk, bk, 0, st, w->sr_pts, w->idx[1], V, n, k, w->sr_dist);
  else hipLaunchKernelGGL(sr_knn<kSrMaxK>, gk, bk, 0, st, w->sr_pts, w->idx[1], V, n, k, w->sr_dist);
  hipLaunchKernelGGL(sr_chunk_sums, dim3(gp), dim3(256), 0, st, w->sr_dist, n, w->sr_csum, w->sr_csq);
  hipLaunchKernelGGL(sr_stats, dim3(1), dim3(64), 0, st, w->sr_csum, w->sr_csq, (n + 63) / 64, V, f.p[0], w->sr_stat);
  hipLaunchKernelGGL(sr_flags, dim3(gp), dim3(256), 0, st, w->pts[c], w->sr_dist, n, w->sr_stat, w->flag);
  w->sr_rows = n;
  return compact(w, st);
}

static bool is_predicate(int t) { return t == SMHIP_FILTER_RANGE || t == SMHIP_FILTER_AXIS_RANGE || t == SMHIP_FILTER_BOUNDING_BOX_REMOVAL; }

hipError_t filt_run_chain(FilterWorkspace* w, hipStream_t st, const smhip_filter_desc_ex* chain, int nf, int* n_out) {
  if (!w || (nf > 0 && !chain)) return hipErrorInvalidValue;
  int k = 0;
  w->sr_rows = -1;
  w->note.clear();
  while (k < nf && w->n > 0) {
    const smhip_filter_desc_ex& f = chain[k];
    const int n = w->n, gp = (n + 255) / 256;
    if (is_predicate(f.type)) {
      PredGroup g{};
      while (k < nf && g.n < kMaxFused && is_predicate(chain[k].type)) {
        Pred& p = g.f[g.n++];
        p.type = chain[k].type; p.axis = chain[k].i[0];
        for (int q = 0; q < 6; ++q) p.p[q] = chain[k].p[q];
        ++k;
      }
      hipLaunchKernelGGL(filt_flags, dim3(gp), dim3(256), 0, st, w->pts[w->cur], n, g, w->flag);
      FCHK(compact(w, st));
    } else if (f.type == SMHIP_FILTER_RANDOM_SAMPLER) {
      ++k;
      if ((double)f.p[0] > 0.999) continue;                                // filter_random_sample.cc:46-53: the float rate against the DOUBLE literal 0.999 (0.999f passes through)
      hipLaunchKernelGGL(filt_sample_flags, dim3(gp), dim3(256), 0, st, n, f.seed, f.p[0], w->flag);
      FCHK(compact(w, st));
    } else if (f.type == SMHIP_FILTER_VOXEL_GRID) {
      ++k;
      const int c = w->cur;
      FCHK(hipMemsetAsync(w->counts + 1, 0, 4, st));
      hipLaunchKernelGGL(filt_voxel_keys, dim3(gp), dim3(256), 0, st, w->pts[c], n, f.p[0], w->keys[0], w->idx[0], w->counts + 1);
      FCHK(voxel_tail(w, st));
    } else if (f.type == SMHIP_FILTER_GROUND_REMOVAL) {
      ++k;
      FCHK(run_ground_removal(w, st, f));
    } else if (f.type == SMHIP_FILTER_GROUND_REMOVAL2) {
      ++k;
      FCHK(run_ground_removal2(w, st, f));
    } else if (f.type == SMHIP_FILTER_RANGE_IMAGE) {
      ++k;
      FCHK(run_range_image(w, st, f));
    } else if (f.type == SMHIP_FILTER_STATISTIC_REMOVAL) {
      ++k;
      FCHK(run_statistic_removal(w, st, f));
    } else {
      return hipErrorInvalidValue;
    }
  }
  if (n_out) *n_out = w->n;
  return hipGetLastError();
}

// ---- a cloud written by a kernel of another unit (smhip_submap.hip) -----------------------------
FilterBuild filt_build_begin(FilterWorkspace* w, hipStream_t st) {
  FilterBuild b{};
  if (!w || hipMemsetAsync(w->counts + 1, 0, 4, st) != hipSuccess) return b;
  b.pts = w->pts[0]; b.fac = w->fac[0]; b.src = w->src[0]; b.keys = w->keys[0]; b.idx = w->idx[0]; b.bad = w->counts + 1;
  return b;
}

hipError_t filt_build_commit(FilterWorkspace* w, hipStream_t st, int n, bool keyed, int* n_out) {
  if (!w || n <= 0 || n > w->cap) return hipErrorInvalidValue;
  w->cur = 0; w->n = n; w->has_index = true;
  if (keyed) FCHK(voxel_tail(w, st));
  else FCHK(hipStreamSynchronize(st));
  if (n_out) *n_out = w->n;
  return hipGetLastError();
}

// ---- MotionCompensation of the current cloud (kernel: motion_comp.hip) ---------------------------
hipError_t filt_motion_compensate(FilterWorkspace* w, hipStream_t st, const MotionCompArgs& a, float4* out) {
  if (!w || !out || w->n <= 0 || w->n > w->cap) return hipErrorInvalidValue;
  const int n = w->n, c = w->cur;
  FCHK(hipMemsetAsync(w->counts + 2, 0, 4, st));
  hipLaunchKernelGGL(filt_motion_comp, dim3((n + 255) / 256), dim3(256), 0, st, w->pts[c], w->fac[c], n, a, out, w->counts + 2);
  FCHK(hipGetLastError());
  return hipMemcpyAsync(w->host_pinned + 3, w->counts + 2, 4, hipMemcpyDeviceToHost, st);
}
bool filt_motion_bad_factor(const FilterWorkspace* w) { return w->host_pinned[3] != 0; }
int32_t* filt_motion_flag_begin(FilterWorkspace* w, hipStream_t st) {
  return w && hipMemsetAsync(w->counts + 2, 0, 4, st) == hipSuccess ? w->counts + 2 : nullptr;
}
hipError_t filt_motion_flag_end(FilterWorkspace* w, hipStream_t st) {
  return hipMemcpyAsync(w->host_pinned + 3, w->counts + 2, 4, hipMemcpyDeviceToHost, st);
}

const float4* filt_points(const FilterWorkspace* w) { return w->pts[w->cur]; }
const float* filt_factors(const FilterWorkspace* w) { return w->fac[w->cur]; }
const int32_t* filt_source_index(const FilterWorkspace* w) { return w->src[w->cur]; }
int filt_count(const FilterWorkspace* w) { return w->n; }
bool filt_has_index(const FilterWorkspace* w) { return w->has_index; }
const char* filt_note(const FilterWorkspace* w) { return w->note.c_str(); }
int filt_statistic_rows(const FilterWorkspace* w) { return w->sr_rows; }
const float* filt_statistic_distance(const FilterWorkspace* w) { return w->sr_dist; }
const double* filt_statistic_stats(const FilterWorkspace* w) { return w->sr_stat; }

}  // namespace smhip
