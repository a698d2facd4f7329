// smhip_icp_information.hip -- the 6x6 information of a point-to-plane alignment at a given transform: kernels and C ABI.
//
// The matcher's normal matrix is rank-deficient exactly where the geometry does not constrain the pose; this unit hands it to the
// back end in the tangent convention of the pose graph's BETWEEN residual (smhip.h, "Pose graph": rotation first, T <- T * [Exp(phi), rho]).
// The matching half is the one-iteration pass smhip_icp_trimmed_score runs (smhip_api.hip: trimmed_pass_range, with every match
// exact); what is new is one pass over the slot's source:
//   information_sums   grid (blocks of 2 048 rows, pairs).  A row streams its source point (16 B), its match and its distance (8 B);
//                      a KEPT row -- d2 finite, d2 <= the pair's limit, a match inside the target -- gathers the matched centred
//                      point and its normal (32 B) and adds J J^T (21 sums) and r^2 in f64; every other row adds nothing and its
//                      match is never used as an index.  Each lane holds the 22 sums, a wave reduces them by DPP, a workgroup
//                      writes ONE row of IcpDev::partials (free once the pass is done: the iteration kernels return on `done`).
//   information_fold   one workgroup per pair adds the pair's rows in index order and writes the smhip_icp_information.
// No floating-point atomics anywhere: the partition is fixed by ns alone and every order of addition is fixed, so two calls --
// and the range call and the single calls -- give the same bits.  Memory-shaped: 24 B per row + 32 B per kept row.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "smhip_context.h"

using namespace smhip_host;

namespace {

constexpr int kInfoThreads = kAccThreads;
constexpr int kInfoItems = kAccItemsSmall;        // rows per thread: a workgroup's 2 048 rows are one row of `partials` (part_stride = acc_blocks)
constexpr int kInfoSums = 22;                     // 21 (H upper, row by row) + sum r^2
constexpr int kInfoCols = 24;                     // + kept + n_finite
static_assert(kInfoCols <= kAccCols, "a workgroup's sums fit a row of IcpDev::partials");
static_assert(kInfoThreads == 256, "information_sums folds exactly four waves (s_red[0..3])");

// v of the lanes a DPP control reads from, 0.0 where the control has no source lane or the row is masked off
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double info_dpp_or_zero(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
// Sum over the wave, left in lane 63 (the reduction of icp_kernels.hip's accumulate: row_shr 1, 2, 4, 8, then row_bcast 15 and 31)
__device__ __forceinline__ double info_wave_sum_to_last(double v) {
  v += info_dpp_or_zero<0x111, 0xf>(v);
  v += info_dpp_or_zero<0x112, 0xf>(v);
  v += info_dpp_or_zero<0x114, 0xf>(v);
  v += info_dpp_or_zero<0x118, 0xf>(v);
  v += info_dpp_or_zero<0x142, 0xa>(v);
  v += info_dpp_or_zero<0x143, 0xc>(v);
  return v;
}

__global__ __launch_bounds__(kInfoThreads) void information_sums(IcpDev b, int first) {
  const int pair = first + (int)blockIdx.y, blk = (int)blockIdx.x;
  const PairState* st = &b.state[pair];
  if (!st->done || st->status != 0) return;                 // the fold reports the status; nothing of this pair's rows is read
  const int ns = min(st->ns, b.ns_cap), nt = min(st->nt, b.nt_cap);
  const int base = blk * (kInfoThreads * kInfoItems);
  if (base >= ns || blk >= b.part_stride) return;
  // T(-mu) * T, row-major, as pose_setup left it: R and t - mu (scalar loads)
  double R[9], tc[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) R[3 * r + c] = st->G[4 * r + c];
    tc[r] = st->G[4 * r + 3];
  }
  const uint32_t limit_key = st->limit_key;
  const size_t so = (size_t)pair * b.ns_cap, to = (size_t)pair * b.nt_cap;
  // the streamed values of the workgroup's rows first, all of them in flight at once; then the kept rows' gathers
  float d[kInfoItems];
  int j[kInfoItems];
  float4 s[kInfoItems];
#pragma unroll
  for (int k = 0; k < kInfoItems; ++k) {
    const int ic = min(base + k * kInfoThreads + (int)threadIdx.x, ns - 1);
    d[k] = b.d2[so + ic];
    j[k] = b.idx[so + ic];
    s[k] = b.src[so + ic];
  }
  bool keep[kInfoItems];
  float4 q[kInfoItems], n[kInfoItems];
  int nkept = 0, nfin = 0;                                  // per wave (uniform)
#pragma unroll
  for (int k = 0; k < kInfoItems; ++k) {
    const bool in = base + k * kInfoThreads + (int)threadIdx.x < ns;
    const uint32_t key = __float_as_uint(d[k]);
    const bool fin = in && key < 0x7f800000u;               // finite and not negative (keys order like the floats)
    keep[k] = fin && key <= limit_key && j[k] >= 0 && j[k] < nt;
    q[k] = make_float4(0, 0, 0, 0); n[k] = make_float4(0, 0, 0, 0);
    if (keep[k]) { q[k] = b.tq[to + j[k]]; n[k] = b.tn[to + j[k]]; }
    nfin += (int)__popcll(__ballot(fin));
    nkept += (int)__popcll(__ballot(keep[k]));
  }
  double acc[kInfoSums];
#pragma unroll
  for (int c = 0; c < kInfoSums; ++c) acc[c] = 0.0;
#pragma unroll
  for (int k = 0; k < kInfoItems; ++k) {
    if (!keep[k]) continue;
    const double x = s[k].x, y = s[k].y, z = s[k].z;
    const double px = fma(R[0], x, fma(R[1], y, fma(R[2], z, tc[0])));      // the moved point, as the iteration kernels form it
    const double py = fma(R[3], x, fma(R[4], y, fma(R[5], z, tc[1])));
    const double pz = fma(R[6], x, fma(R[7], y, fma(R[8], z, tc[2])));
    const double nx = n[k].x, ny = n[k].y, nz = n[k].z;
    const double r = (px - (double)q[k].x) * nx + (py - (double)q[k].y) * ny + (pz - (double)q[k].z) * nz;
    const double mx = fma(R[0], nx, fma(R[3], ny, R[6] * nz));              // m = R^T n
    const double my = fma(R[1], nx, fma(R[4], ny, R[7] * nz));
    const double mz = fma(R[2], nx, fma(R[5], ny, R[8] * nz));
    const double J[6] = {y * mz - z * my, z * mx - x * mz, x * my - y * mx, mx, my, mz};   // [s x m ; m]
    int c = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int e = a; e < 6; ++e) acc[c++] += J[a] * J[e];
    acc[21] += r * r;
  }
  __shared__ double s_red[kInfoThreads / 64][kInfoCols];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < kInfoSums; ++c) acc[c] = info_wave_sum_to_last(acc[c]);
  if (lane == 63) {
#pragma unroll
    for (int c = 0; c < kInfoSums; ++c) s_red[wave][c] = acc[c];
    s_red[wave][22] = (double)nkept;
    s_red[wave][23] = (double)nfin;
  }
  __syncthreads();
  if (threadIdx.x < kInfoCols)
    b.partials[((size_t)pair * b.part_stride + blk) * kAccCols + threadIdx.x] =
        ((s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + s_red[2][threadIdx.x]) + s_red[3][threadIdx.x];
}

__global__ __launch_bounds__(64) void information_fold(IcpDev b, int first, int npairs, smhip_icp_information* out) {
  const int k = (int)blockIdx.x;
  if (k >= npairs) return;
  const int pair = first + k;
  const PairState* st = &b.state[pair];
  __shared__ double s_tot[kInfoCols];
  const bool ok = st->done && st->status == 0;
  const int ns = min(st->ns, b.ns_cap);
  const int rows = ok ? min((ns + kInfoThreads * kInfoItems - 1) / (kInfoThreads * kInfoItems), b.part_stride) : 0;
  if (threadIdx.x < kInfoCols) {
    double t = 0.0;
    for (int r = 0; r < rows; ++r) t += b.partials[((size_t)pair * b.part_stride + r) * kAccCols + threadIdx.x];   // index order
    s_tot[threadIdx.x] = t;
  }
  __syncthreads();
  smhip_icp_information* o = out + k;
  if (threadIdx.x < 36) {
    const int a = min((int)threadIdx.x / 6, (int)threadIdx.x % 6), e = max((int)threadIdx.x / 6, (int)threadIdx.x % 6);
    o->H[threadIdx.x] = s_tot[a * 6 - a * (a - 1) / 2 + (e - a)];
  }
  if (threadIdx.x == 0) {
    o->sum_r2 = s_tot[21];
    o->limit_d2 = ok ? (double)__uint_as_float(st->limit_key) : 0.0;
    o->kept = (int32_t)s_tot[22];
    o->n_finite = (int32_t)s_tot[23];
    o->status = st->done ? st->status : SMHIP_ERR_HIP;
    o->reserved = 0;
  }
}

smhip_status information_range(smhip_context* h, int first, int npairs, const double* Ts, float ratio, smhip_icp_information* out) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  if (npairs < 1 || first < 0 || first + npairs > h->dev.slots) { h->err = "slot out of range"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (!Ts || !out) { h->err = "icp information: T and out must not be NULL"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (!(ratio >= 0.f && ratio <= 1.f)) { h->err = "dist_outlier_ratio must be in [0, 1]"; return SMHIP_ERR_INVALID_ARGUMENT; }
  int ns_max = 0;
  for (int p = first; p < first + npairs; ++p) {
    if (h->ns[p] <= 0 || h->nt[p] <= 0) { h->err = "icp information before SetInputSource/SetInputTarget"; return SMHIP_ERR_NOT_READY; }
    if (!h->has_normals[p]) { h->err = "icp information: the target has no normals"; return SMHIP_ERR_NO_NORMALS; }
    ns_max = std::max(ns_max, h->ns[p]);
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->info_dev) {
    smhip_status a = dev_alloc(h, &h->info_dev, (size_t)h->dev.slots);
    if (a) return a;
  }
  std::vector<smhip_icp_stats> stats((size_t)npairs);
  const smhip_status s = trimmed_pass_range(h, first, npairs, Ts, ratio, stats.data());
  bool pair_failed = false;
  for (const smhip_icp_stats& st : stats) pair_failed = pair_failed || st.status != SMHIP_OK;
  if (s != SMHIP_OK && !pair_failed) return s;              // the call failed, not one of its pairs
  const int blocks = (ns_max + kInfoThreads * kInfoItems - 1) / (kInfoThreads * kInfoItems);
  // a workgroup's sums are one row of `partials`: part_stride = ceil(ns_cap / 2 048) rows a pair.  Fewer would drop rows of the source
  // (the kernels' own `blk < part_stride` guards only keep the stores in bounds), so that is refused, not clamped.
  if (blocks > (int)h->dev.part_stride) { h->err = "icp information: the source needs more partial rows than the handle holds"; return SMHIP_ERR_INVALID_ARGUMENT; }
  hipLaunchKernelGGL(information_sums, dim3(blocks, npairs), dim3(kInfoThreads), 0, h->stream, h->dev, first);
  hipLaunchKernelGGL(information_fold, dim3(npairs), dim3(64), 0, h->stream, h->dev, first, npairs, h->info_dev);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(out, h->info_dev, sizeof(smhip_icp_information) * (size_t)npairs, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return s;
}

}  // namespace

extern "C" {

smhip_status smhip_icp_information_at(smhip_handle h, int slot, const double T[16], float dist_outlier_ratio, smhip_icp_information* out) {
  return information_range(h, slot, 1, T, dist_outlier_ratio, out);
}

smhip_status smhip_icp_information_range(smhip_handle h, int first_slot, int npairs, const double* Ts, float dist_outlier_ratio,
                                         smhip_icp_information* out) {
  return information_range(h, first_slot, npairs, Ts, dist_outlier_ratio, out);
}

}  // extern "C"
