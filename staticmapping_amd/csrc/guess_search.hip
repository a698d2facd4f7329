// guess_search.hip -- the correlative guess search (DESIGN.md §6 "Guess search", restated in tests/guess_search_ref.py): kernels
// and C ABI.  Every transform of a window around a guess is scored by how many sampled source points land in an occupied voxel of
// the target; the best one is what LoopDetector::CloseLoop starts its ICP from when the drifted poses are too far off for it.
//
// One call, on the handle's stream, plain launches:
//   guess_search_bounds      min / max of floor(p / res) over the target's finite rows (integer atomics: order-free), the count of
//                            finite rows and a flag for a coordinate that does not fit
//   (the host reads the box: the bitmap's layout, its capacity check and the workspace follow from it)
//   guess_search_occupancy   one bit per occupied voxel of the box, atomicOr
//   guess_search_voxels      per yaw, every sampled source point's voxel relative to the box origin, packed into 64 bits
//   guess_search_score       a thread owns one (i, j, k) offset of one yaw and tests that yaw's source voxels one after the other;
//                            the voxel's address is wave-uniform (scalar loads), neighbouring lanes take neighbouring i, so a wave
//                            reads one or two dwords of a bitmap row; the score volume is written once with plain stores
//   guess_search_pick        one workgroup: rule 7 over the stored volume under a total order (so the fold's shape does not
//                            matter), the score at the guess, then runner_up_score
// Rows are dropped and the source sampled (rules 1 and 2, integers only) while the clouds are staged for upload: the host touches
// every row once there anyway.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "smhip_context.h"
#include "guess_search_plan.h"

using namespace smhip_host;
namespace gs = smhip_guess_search;

namespace {

constexpr int kGsThreads = 256;
constexpr int kGsPickThreads = 1024;
// ctl words: 0-2 box min, 3-5 box max, 6 finite target rows, 7 a voxel coordinate does not fit, 8 best score, 9 best flat index,
// 10 score at the guess, 11 runner-up score
constexpr int kGsCtl = 16;

__device__ __forceinline__ bool gs_finite(const float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// floor(p / res): the IEEE quotient, then floorf.  false when the voxel does not fit the index type (or is not a number).
__device__ __forceinline__ bool gs_voxel(float p, float res, int* v) {
  const float f = floorf(__fdiv_rn(p, res));
  if (!(fabsf(f) < (float)gs::kMaxVoxel)) return false;
  *v = (int)f;
  return true;
}

__global__ __launch_bounds__(kGsThreads) void guess_search_bounds(const float4* __restrict__ pts, int n, float res, int32_t* __restrict__ ctl) {
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN}, cnt = 0;
  bool bad = false;
  for (int i = blockIdx.x * kGsThreads + threadIdx.x; i < n; i += gridDim.x * kGsThreads) {
    const float4 p = pts[i];
    if (!gs_finite(p)) continue;
    ++cnt;
    int v[3];
    if (!gs_voxel(p.x, res, &v[0]) || !gs_voxel(p.y, res, &v[1]) || !gs_voxel(p.z, res, &v[2])) { bad = true; continue; }
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo[c] = min(lo[c], v[c]); hi[c] = max(hi[c], v[c]); }
  }
  __shared__ int s_lo[3], s_hi[3], s_cnt, s_bad;
  if (threadIdx.x == 0) { for (int c = 0; c < 3; ++c) { s_lo[c] = INT_MAX; s_hi[c] = INT_MIN; } s_cnt = 0; s_bad = 0; }
  __syncthreads();
  if (cnt) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { atomicMin(&s_lo[c], lo[c]); atomicMax(&s_hi[c], hi[c]); }
    atomicAdd(&s_cnt, cnt);
  }
  if (bad) s_bad = 1;
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) {
    for (int c = 0; c < 3; ++c) { atomicMin(&ctl[c], s_lo[c]); atomicMax(&ctl[3 + c], s_hi[c]); }
    atomicAdd(&ctl[6], s_cnt);
    if (s_bad) ctl[7] = 1;
  }
}

struct GsBox { int ox, oy, oz, nx, ny, nz, row_words; };

__global__ __launch_bounds__(kGsThreads) void guess_search_occupancy(const float4* __restrict__ pts, int n, float res, GsBox b, uint32_t* __restrict__ bitmap) {
  const int i = blockIdx.x * kGsThreads + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  if (!gs_finite(p)) return;
  int v[3];
  if (!gs_voxel(p.x, res, &v[0]) || !gs_voxel(p.y, res, &v[1]) || !gs_voxel(p.z, res, &v[2])) return;
  const int x = v[0] - b.ox, y = v[1] - b.oy, z = v[2] - b.oz;
  if ((unsigned)x >= (unsigned)b.nx || (unsigned)y >= (unsigned)b.ny || (unsigned)z >= (unsigned)b.nz) return;   // (the box came from these rows)
  atomicOr(&bitmap[((size_t)z * b.ny + y) * b.row_words + (x >> 5)], 1u << (x & 31));
}

// bpy workgroups per yaw, yaw-major in blockIdx.x (a grid's y could not hold 2^20 yaws).  yaw12: r00 r01 r02 r10 .. r22 tx ty tz as float.  q = ((r0 x + r1 y) + r2 z) + t, every product and sum
// rounded on its own.
__global__ __launch_bounds__(kGsThreads) void guess_search_voxels(const float4* __restrict__ src, int m, const float* __restrict__ yaw12, float res, GsBox b,
                                                                 int half_xy, int half_z, int bpy, unsigned long long* __restrict__ vox, int32_t* __restrict__ ctl) {
#pragma clang fp contract(off)
  const int yaw = blockIdx.x / bpy, p = (blockIdx.x % bpy) * kGsThreads + threadIdx.x;
  if (p >= m) return;
  const float* T = yaw12 + 12 * yaw;
  const float4 s = src[p];
  const float qx = ((T[0] * s.x + T[1] * s.y) + T[2] * s.z) + T[9];
  const float qy = ((T[3] * s.x + T[4] * s.y) + T[5] * s.z) + T[10];
  const float qz = ((T[6] * s.x + T[7] * s.y) + T[8] * s.z) + T[11];
  int w[3];
  unsigned long long out = gs::kNeverVoxel;
  if (!gs_voxel(qx, res, &w[0]) || !gs_voxel(qy, res, &w[1]) || !gs_voxel(qz, res, &w[2])) {
    ctl[7] = 1;                                                        // (every writer stores the same value)
  } else {
    const long long rx = (long long)w[0] - b.ox, ry = (long long)w[1] - b.oy, rz = (long long)w[2] - b.oz;
    if (rx >= -half_xy && rx < (long long)b.nx + half_xy && ry >= -half_xy && ry < (long long)b.ny + half_xy && rz >= -half_z && rz < (long long)b.nz + half_z)
      out = gs::PackVoxel((int)rx, (int)ry, (int)rz);
  }
  vox[(size_t)yaw * m + p] = out;
}

// bpy workgroups per yaw, yaw-major in blockIdx.x; one offset per thread, i fastest.  The loop's loads of vox[] have a wave-uniform
// address.  No branch in the loop: a lane whose voxel falls outside the box reads word 0 (there is always one) and adds nothing, so the
// loads of several iterations are in flight together.  The bitmap is read from global memory (it stays in L2): a variant that first
// copied it to LDS was measured and not kept (DESIGN.md §6 "Guess search").
__global__ __launch_bounds__(kGsThreads) void guess_search_score(const unsigned long long* __restrict__ vox, int m, const uint32_t* __restrict__ bitmap, GsBox b,
                                                                int half_xy, int half_z, int nxy, int n_offsets, int bpy, int32_t* __restrict__ volume) {
  const int yaw = blockIdx.x / bpy, o = (blockIdx.x % bpy) * kGsThreads + threadIdx.x;
  if (o >= n_offsets) return;
  const int di = o % nxy - half_xy, dj = (o / nxy) % nxy - half_xy, dk = o / (nxy * nxy) - half_z;
  const unsigned long long* v = vox + (size_t)yaw * m;
  unsigned score = 0;
#pragma unroll 8
  for (int p = 0; p < m; ++p) {
    int sx, sy, sz;
    gs::UnpackVoxel(v[p], &sx, &sy, &sz);
    const int x = sx + di, y = sy + dj, z = sz + dk;
    // all ones when the voxel is inside the box, else 0 -- by arithmetic, so that the load stays unconditional
    const unsigned inside = 0u - (unsigned)(((unsigned)x < (unsigned)b.nx) & ((unsigned)y < (unsigned)b.ny) & ((unsigned)z < (unsigned)b.nz));
    const unsigned at = (unsigned)((z * b.ny + y) * b.row_words + (x >> 5)) & inside;            // < 2^23 words
    score += (bitmap[at] >> (x & 31)) & inside & 1u;
  }
  volume[(size_t)yaw * n_offsets + o] = (int32_t)score;
}

// One workgroup.  Every thread folds its candidates under gs::Better, a total order, then the workgroup folds the threads' picks.
__global__ __launch_bounds__(kGsPickThreads) void guess_search_pick(const int32_t* __restrict__ volume, gs::Window w, int32_t* __restrict__ ctl) {
  __shared__ int s_score[kGsPickThreads], s_flat[kGsPickThreads];
  const int t = threadIdx.x, n = (int)w.n_candidates;
  int bs = -1, bf = 0;                                                   // (-1 loses against every score: a thread with no candidate)
  for (int f = t; f < n; f += kGsPickThreads) {
    const int s = volume[f];
    bool take = s > bs;
    if (s == bs) take = gs::Better(s, gs::Decode(f, w), bs, gs::Decode(bf, w));
    bs = take ? s : bs;
    bf = take ? f : bf;
  }
  s_score[t] = bs; s_flat[t] = bf;
  __syncthreads();
  for (int off = kGsPickThreads / 2; off > 0; off >>= 1) {
    if (t < off) {
      const int so = s_score[t + off], fo = s_flat[t + off], sm = s_score[t], fm = s_flat[t];
      bool take = so > sm;
      if (so == sm && so >= 0) take = gs::Better(so, gs::Decode(fo, w), sm, gs::Decode(fm, w));
      if (take) { s_score[t] = so; s_flat[t] = fo; }
    }
    __syncthreads();
  }
  const int best_flat = s_flat[0], best_score = s_score[0];
  __syncthreads();
  const gs::Candidate best = gs::Decode(best_flat, w);
  int r = 0;
  for (int f = t; f < n; f += kGsPickThreads) {
    const int s = volume[f];
    if (s > r && gs::Apart(best, gs::Decode(f, w))) r = s;
  }
  s_score[t] = r;
  __syncthreads();
  for (int off = kGsPickThreads / 2; off > 0; off >>= 1) {
    if (t < off) s_score[t] = max(s_score[t], s_score[t + off]);
    __syncthreads();
  }
  if (t == 0) {
    gs::Candidate zero;
    ctl[8] = best_score; ctl[9] = best_flat; ctl[10] = volume[gs::Encode(zero, w)]; ctl[11] = s_score[0];
  }
}

}  // namespace

// what a handle keeps for the search: grown to fit a call, never shrunk
struct smhip_guess_search_state {
  float4* tgt = nullptr; float4* src = nullptr;
  uint32_t* bitmap = nullptr;
  unsigned long long* vox = nullptr;
  int32_t* volume = nullptr;
  float* yaw = nullptr;
  int32_t* ctl = nullptr;
  int32_t* pinned_ctl = nullptr;
  float* pinned_yaw = nullptr;
  size_t tgt_cap = 0, src_cap = 0, bitmap_cap = 0, vox_cap = 0, volume_cap = 0, yaw_cap = 0, pinned_yaw_cap = 0;   // in elements
  bool have_last = false;          // what smhip_guess_search_last can return
  gs::Window window;
  gs::Bitmap box;
  int m = 0;
};

namespace {

template <typename T>
smhip_status gs_grow(smhip_context* h, T** p, size_t* cap, size_t need) {
  if (need <= *cap) return SMHIP_OK;
  if (*p) { HIPCHK(h, hipFree(*p)); *p = nullptr; *cap = 0; }
  void* v = nullptr;
  HIPCHK(h, hipMalloc(&v, need * sizeof(T)));
  *p = reinterpret_cast<T*>(v); *cap = need;
  return SMHIP_OK;
}

smhip_status gs_refuse(smhip_context* h, gs::Refusal r, const std::string& why) {
  h->err = "guess search: " + why;
  return r == gs::kCapacity ? SMHIP_ERR_CAPACITY : SMHIP_ERR_INVALID_ARGUMENT;
}

// rows with a finite x, y and z go to `out` as float4, in order; the count
size_t gs_stage(const float* rows, int stride, long long n, float4* out) {
  size_t k = 0;
  for (long long i = 0; i < n; ++i) {
    const float* r = rows + (size_t)stride * i;
    if (std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2])) out[k++] = make_float4(r[0], r[1], r[2], r[3]);
  }
  return k;
}

}  // namespace

extern "C" {

void smhip_internal_free_guess_search(smhip_context* h) {
  smhip_guess_search_state* st = h->guess_search;
  if (!st) return;
  for (void* p : {(void*)st->tgt, (void*)st->src, (void*)st->bitmap, (void*)st->vox, (void*)st->volume, (void*)st->yaw, (void*)st->ctl})
    if (p) (void)hipFree(p);
  if (st->pinned_ctl) (void)hipHostFree(st->pinned_ctl);
  if (st->pinned_yaw) (void)hipHostFree(st->pinned_yaw);
  delete st;
  h->guess_search = nullptr;
}

void smhip_guess_search_default_options(smhip_guess_search_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->resolution = 0.5f; o->max_source_points = 4096;
  o->half_xy = 20; o->half_z = 2; o->yaw_steps = 10;
  o->yaw_step = 2.0 * M_PI / 180.0;
}

smhip_status smhip_guess_search_f32(smhip_handle h, const float* target, int n_target, int target_stride, const float* source, int n_source,
                                    int source_stride, const double* guess, const smhip_guess_search_options* opts, smhip_guess_search_result* result) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  gs::Window w;
  std::string why;
  const bool pointers = target && source && guess && opts && result;
  const gs::Refusal r = gs::Check(pointers, target_stride, source_stride, n_target, n_source, pointers ? (double)opts->resolution : 1.0,
                                  pointers ? opts->half_xy : 0, pointers ? opts->half_z : 0, pointers ? opts->yaw_steps : 0,
                                  pointers ? opts->yaw_step : 0.0, pointers ? opts->max_source_points : 1, guess,
                                  std::max(h->dev.ns_cap, h->dev.nt_cap), &w, &why);
  if (r != gs::kOk) return gs_refuse(h, r, why);
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->guess_search) {
    auto* st = new smhip_guess_search_state;
    if (hipMalloc(reinterpret_cast<void**>(&st->ctl), sizeof(int32_t) * kGsCtl) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&st->pinned_ctl), sizeof(int32_t) * 2 * kGsCtl) != hipSuccess) {
      if (st->ctl) (void)hipFree(st->ctl);
      delete st;
      h->err = "guess search: allocation failed";
      return SMHIP_ERR_HIP;
    }
    h->guess_search = st;
  }
  smhip_guess_search_state* st = h->guess_search;
  hipStream_t s = h->stream;
  const float res = opts->resolution;
  st->have_last = false;
  HIPCHK(h, hipStreamSynchronize(s));                                    // the staging area is the handle's

  // rules 1 and 2 while staging: the target's finite rows, then the source's, sampled in place
  const size_t cap = (size_t)std::max(h->dev.ns_cap, h->dev.nt_cap);
  float4* stage_t = h->stage;
  float4* stage_s = h->stage + cap;
  const size_t nt = gs_stage(target, target_stride, n_target, stage_t);
  const size_t ns = gs_stage(source, source_stride, n_source, stage_s);
  if (nt == 0 || ns == 0) return gs_refuse(h, gs::kInvalid, "a cloud has no row with finite coordinates");
  const long long M = opts->max_source_points;
  const int m = (int)gs::SampleCount((long long)ns, M);
  if ((long long)ns > M)
    for (long long k = 0; k < m; ++k) stage_s[k] = stage_s[gs::SampleRow(k, (long long)ns, M)];   // SampleRow(k) >= k: never reads a written row

  smhip_status e = gs_grow(h, &st->tgt, &st->tgt_cap, nt);
  if (!e) e = gs_grow(h, &st->src, &st->src_cap, (size_t)m);
  if (!e) e = gs_grow(h, &st->volume, &st->volume_cap, (size_t)w.n_candidates);
  if (!e) e = gs_grow(h, &st->vox, &st->vox_cap, (size_t)w.nyaw * m);
  if (!e) e = gs_grow(h, &st->yaw, &st->yaw_cap, (size_t)12 * w.nyaw);
  if (e) return e;
  if ((size_t)12 * w.nyaw > st->pinned_yaw_cap) {
    if (st->pinned_yaw) { (void)hipHostFree(st->pinned_yaw); st->pinned_yaw = nullptr; st->pinned_yaw_cap = 0; }
    HIPCHK(h, hipHostMalloc(reinterpret_cast<void**>(&st->pinned_yaw), sizeof(float) * 12 * w.nyaw));
    st->pinned_yaw_cap = (size_t)12 * w.nyaw;
  }
  for (int a = -w.yaw_steps; a <= w.yaw_steps; ++a) {                     // rule 4: double on the host, cast to float
    double T[12];
    gs::YawTransform(guess, a * opts->yaw_step, T);
    for (int c = 0; c < 12; ++c) st->pinned_yaw[12 * (a + w.yaw_steps) + c] = (float)T[c];
  }
  int32_t* pc = st->pinned_ctl;
  for (int c = 0; c < kGsCtl; ++c) pc[c] = 0;
  pc[0] = pc[1] = pc[2] = INT_MAX; pc[3] = pc[4] = pc[5] = INT_MIN;
  HIPCHK(h, hipMemcpyAsync(st->ctl, pc, sizeof(int32_t) * kGsCtl, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(st->tgt, stage_t, sizeof(float4) * nt, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(st->src, stage_s, sizeof(float4) * (size_t)m, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(st->yaw, st->pinned_yaw, sizeof(float) * 12 * w.nyaw, hipMemcpyHostToDevice, s));
  const int tb = (int)std::min<size_t>(1024, (nt + kGsThreads - 1) / kGsThreads);
  hipLaunchKernelGGL(guess_search_bounds, dim3(tb), dim3(kGsThreads), 0, s, st->tgt, (int)nt, res, st->ctl);
  HIPCHK(h, hipGetLastError());
  int32_t* back = st->pinned_ctl + kGsCtl;
  HIPCHK(h, hipMemcpyAsync(back, st->ctl, sizeof(int32_t) * kGsCtl, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  if (back[7]) return gs_refuse(h, gs::kCapacity, "a target voxel coordinate does not fit the index type");
  if (back[6] < 1) return gs_refuse(h, gs::kInvalid, "the target has no row with finite coordinates");
  gs::Bitmap box;
  const gs::Refusal rb = gs::MakeBitmap(back, back + 3, w.half_xy, w.half_z, &box, &why);
  if (rb != gs::kOk) return gs_refuse(h, rb, why);
  e = gs_grow(h, &st->bitmap, &st->bitmap_cap, (size_t)box.words);
  if (e) return e;
  const GsBox b{box.origin[0], box.origin[1], box.origin[2], box.extent[0], box.extent[1], box.extent[2], box.row_words};
  HIPCHK(h, hipMemsetAsync(st->bitmap, 0, sizeof(uint32_t) * (size_t)box.words, s));
  hipLaunchKernelGGL(guess_search_occupancy, dim3((unsigned)((nt + kGsThreads - 1) / kGsThreads)), dim3(kGsThreads), 0, s, st->tgt, (int)nt, res, b, st->bitmap);
  // (both grids fit: at most 2^10 workgroups per yaw x 2^20 yaws here, 2^25 / 256 + 2^20 there)
  const int vb = (m + kGsThreads - 1) / kGsThreads;
  hipLaunchKernelGGL(guess_search_voxels, dim3((unsigned)vb * w.nyaw), dim3(kGsThreads), 0, s, st->src, m, st->yaw, res, b, w.half_xy, w.half_z, vb, st->vox,
                     st->ctl);
  const int n_off = (int)w.n_offsets, sb = (n_off + kGsThreads - 1) / kGsThreads;
  hipLaunchKernelGGL(guess_search_score, dim3((unsigned)sb * w.nyaw), dim3(kGsThreads), 0, s, st->vox, m, st->bitmap, b, w.half_xy, w.half_z, w.nxy, n_off,
                     sb, st->volume);
  hipLaunchKernelGGL(guess_search_pick, dim3(1), dim3(kGsPickThreads), 0, s, st->volume, w, st->ctl);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(back, st->ctl, sizeof(int32_t) * kGsCtl, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  if (back[7]) return gs_refuse(h, gs::kCapacity, "a source voxel coordinate does not fit the index type");
  st->have_last = true; st->window = w; st->box = box; st->m = m;

  const gs::Candidate c = gs::Decode(back[9], w);
  double T[12];
  gs::YawTransform(guess, c.a * opts->yaw_step, T);
  smhip_guess_search_result out;
  std::memset(&out, 0, sizeof(out));
  for (int row = 0; row < 3; ++row)
    for (int col = 0; col < 3; ++col) out.transform[4 * col + row] = T[3 * row + col];
  out.transform[12] = guess[12] + (double)res * c.i;
  out.transform[13] = guess[13] + (double)res * c.j;
  out.transform[14] = guess[14] + (double)res * c.k;
  out.transform[15] = 1.0;
  out.best_score = back[8]; out.guess_score = back[10]; out.runner_up_score = back[11];
  out.n_source_used = m; out.n_candidates = (int32_t)w.n_candidates;
  out.best_yaw = c.a; out.best_i = c.i; out.best_j = c.j; out.best_k = c.k;
  *result = out;
  return SMHIP_OK;
}

smhip_status smhip_guess_search_last(smhip_handle h, int32_t* volume, int volume_len, int32_t* origin3, int32_t* extent3, int32_t* source_voxels,
                                     int voxels_len) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  smhip_guess_search_state* st = h->guess_search;
  if (!st || !st->have_last) { h->err = "guess search: no search has completed on this handle"; return SMHIP_ERR_NOT_READY; }
  const long long nv = (long long)st->window.nyaw * st->m;
  if ((volume && volume_len != st->window.n_candidates) || (source_voxels && voxels_len != 3 * nv)) {
    h->err = "guess search: volume_len must equal n_candidates and voxels_len 3 x yaws x n_source_used of the last call";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<unsigned long long> packed;
  if (volume) HIPCHK(h, hipMemcpyAsync(volume, st->volume, sizeof(int32_t) * (size_t)volume_len, hipMemcpyDeviceToHost, h->stream));
  if (source_voxels) {
    packed.resize((size_t)nv);
    HIPCHK(h, hipMemcpyAsync(packed.data(), st->vox, sizeof(unsigned long long) * (size_t)nv, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t p = 0; p < packed.size(); ++p) {
    int32_t* o = source_voxels + 3 * p;
    if (packed[p] == gs::kNeverVoxel) { o[0] = o[1] = o[2] = INT32_MIN; continue; }
    int rx, ry, rz;
    gs::UnpackVoxel(packed[p], &rx, &ry, &rz);
    o[0] = rx + st->box.origin[0]; o[1] = ry + st->box.origin[1]; o[2] = rz + st->box.origin[2];
  }
  for (int c = 0; c < 3; ++c) {
    if (origin3) origin3[c] = st->box.origin[c];
    if (extent3) extent3[c] = st->box.extent[c];
  }
  return SMHIP_OK;
}

}  // extern "C"
