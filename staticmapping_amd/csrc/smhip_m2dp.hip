// smhip_m2dp.hip -- descriptor::M2dp (the reference's descriptor/m2dp.{h,cc}) on the device: kernels and C ABI.
//
// setInputCloud (m2dp.cc:122-149) reads every point of a submap cloud p*q times.  Here the cloud stays where it is (an uploaded
// scan, or the filter workspace's current cloud) and one submission on the handle's stream computes the descriptor, with no host
// step between the stages:
//   m2dp_sums / m2dp_mean / m2dp_cov   f64 moments of the f32 rows: a partial per workgroup, folded in index order, so two device
//                                      calls give the same bits (the order, and the fused multiply-adds the compiler forms in
//                                      the centred products, are the device's own: the numpy restatement agrees to ~1e-15
//                                      relative, not bit for bit); a row with a non-finite coordinate sets a flag
//   m2dp_axes                          the 3x3 symmetric eigenproblem (cyclic Jacobi, f64, one lane) and the sign rule
//   m2dp_project                       preProcess (:45-70): V^T (x - mean) in f64 cast to float, the float getLength test (:32-35).
//                                      No compaction: a dropped row adds nothing to the histogram
//   m2dp_hist                          singleViewProcess (:72-120) for every view: integer LDS atomics into the workgroup's copy
//                                      of its views, then integer global atomics into A -- order-free
//   m2dp_gram / m2dp_descriptor        G = A A^T exactly (int64 -> f64), cyclic Jacobi in f64 on one workgroup, u1, v1 = A^T u1 /
//                                      sigma1, the sign rule, the descriptor as float
// What pcl::PCA and Eigen::JacobiSVD leave open is defined in DESIGN.md §6 ("M2DP") and restated in tests/m2dp_ref.py.
//
// The histogram workgroup keeps only the angular bins a sample can reach.  Both projected coordinates are absolute values
// (.norm() of a 1x1 product, :100-101), so atan2 is never above pi/2 and t_index <= t/4: of the l*t columns of a view only
// l*(t/4+1) are ever counted.  At the defaults that is 64 views x 32 x 5 x 4 B = 40 KiB for ALL views, so every point is read
// once and its projected coordinates stay in registers for the 64 views; a workgroup whose views do not fit 40 KiB takes a slice
// of them through blockIdx.y.  (The alternatives: all 128 KiB of A in LDS leaves one workgroup per CU; a slice of 16 full-width
// views is 32 KiB but reads every point four times.  40 KiB leaves four workgroups of 512 threads per CU, the wave limit.)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "smhip_context.h"

using namespace smhip_host;

namespace {

constexpr int kMThreads = 256;             // moments, projection
constexpr int kMParts = 256;               // partial sums per reduction
constexpr int kMHistThreads = 512;
constexpr int kMHistBlocks = 256;          // at most this many workgroups share the points (each flushes its copy once)
constexpr int kMSliceCells = 10240;        // int32 counters of a histogram workgroup: 40 KiB
constexpr int kMMaxViews = 64;             // p * q: G and the rotations of one Jacobi step live in one workgroup's LDS
constexpr int kMMaxCols = 8192;            // l * t: a row of A in LDS (m2dp_gram)
constexpr int kMDescThreads = 1024;
constexpr int kMMaxSweeps = 30;

// doubles of the state, by offset
constexpr int kDSum = 0, kDCov = kDSum + 3 * kMParts, kDMean = kDCov + 6 * kMParts, kDAxes = kDMean + 3,
              kDG = kDAxes + 9, kDV = kDG + kMMaxViews * kMMaxViews, kDTotal = kDV + kMMaxViews * kMMaxViews;
// ctl words: 0 = a row is not finite, 1 = kept rows, 2 = sigma1 is zero, 3 = Jacobi sweeps run
constexpr int kCtl = 4;

__device__ __forceinline__ bool m2dp_finite(const float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// the workgroup's fold: 256 values halved in LDS, a fixed order
template <int C>
__device__ __forceinline__ void m2dp_block_fold(double (&v)[C], double* out) {
  __shared__ double s[C][kMThreads];
  const int t = threadIdx.x;
#pragma unroll
  for (int c = 0; c < C; ++c) s[c][t] = v[c];
  __syncthreads();
  for (int off = kMThreads / 2; off > 0; off >>= 1) {
    if (t < off) {
#pragma unroll
      for (int c = 0; c < C; ++c) s[c][t] = s[c][t] + s[c][t + off];
    }
    __syncthreads();
  }
  if (t < C) out[t] = s[t][0];
}

__global__ __launch_bounds__(kMThreads) void m2dp_sums(const float4* __restrict__ pts, int n, double* __restrict__ dbl, int32_t* __restrict__ ctl) {
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = blockIdx.x * kMThreads + threadIdx.x; i < n; i += gridDim.x * kMThreads) {
    const float4 p = pts[i];
    if (!m2dp_finite(p)) { ctl[0] = 1; continue; }                 // (every writer stores the same value)
    v[0] += (double)p.x; v[1] += (double)p.y; v[2] += (double)p.z;
  }
  m2dp_block_fold<3>(v, dbl + kDSum + 3 * blockIdx.x);
}

__global__ void m2dp_mean(int parts, int n, double* __restrict__ dbl) {
  const int c = threadIdx.x;
  if (c >= 3) return;
  double s = 0.0;
  for (int b = 0; b < parts; ++b) s += dbl[kDSum + 3 * b + c];
  dbl[kDMean + c] = s / (double)n;       // (n counts skipped non-finite rows too: such a call is refused afterwards, its mean is never used)
}

__global__ __launch_bounds__(kMThreads) void m2dp_cov(const float4* __restrict__ pts, int n, double* __restrict__ dbl) {
  const double mx = dbl[kDMean], my = dbl[kDMean + 1], mz = dbl[kDMean + 2];
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = blockIdx.x * kMThreads + threadIdx.x; i < n; i += gridDim.x * kMThreads) {
    const float4 p = pts[i];
    if (!m2dp_finite(p)) continue;
    const double x = (double)p.x - mx, y = (double)p.y - my, z = (double)p.z - mz;
    v[0] += x * x; v[1] += x * y; v[2] += x * z; v[3] += y * y; v[4] += y * z; v[5] += z * z;
  }
  m2dp_block_fold<6>(v, dbl + kDCov + 6 * blockIdx.x);
}

// tan, cos, sin of the Jacobi rotation that zeroes a_pq
__device__ __forceinline__ void m2dp_rotation(double app, double aqq, double apq, double& c, double& s) {
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  c = 1.0 / sqrt(t * t + 1.0);
  s = t * c;
}

// one lane: covariance = fold of the partials / (n - 1), its eigenvectors by cyclic Jacobi, eigenvalues descending, each of the
// first two axes signed so that its largest-magnitude component is positive (ties: the lowest index), third = first x second
__global__ void m2dp_axes(int parts, int n, double* __restrict__ dbl) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double c6[6] = {0, 0, 0, 0, 0, 0};
  for (int b = 0; b < parts; ++b)
    for (int k = 0; k < 6; ++k) c6[k] += dbl[kDCov + 6 * b + k];
  const double d = (double)(n - 1);
  double a[3][3] = {{c6[0] / d, c6[1] / d, c6[2] / d}, {c6[1] / d, c6[3] / d, c6[4] / d}, {c6[2] / d, c6[4] / d, c6[5] / d}};
  double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  const double scale = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]);
  for (int sweep = 0; sweep < 50; ++sweep) {
    if (fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[1][2]) <= 1.0e-22 * scale) break;
    for (int pr = 0; pr < 3; ++pr) {
      const int p = pr == 2 ? 1 : 0, q = pr == 0 ? 1 : 2;
      if (a[p][q] == 0.0) continue;
      double c, s;
      m2dp_rotation(a[p][p], a[q][q], a[p][q], c, s);
      for (int k = 0; k < 3; ++k) {
        const double kp = a[k][p], kq = a[k][q];
        a[k][p] = c * kp - s * kq; a[k][q] = s * kp + c * kq;
        const double vp = v[k][p], vq = v[k][q];
        v[k][p] = c * vp - s * vq; v[k][q] = s * vp + c * vq;
      }
      for (int k = 0; k < 3; ++k) {
        const double pk = a[p][k], qk = a[q][k];
        a[p][k] = c * pk - s * qk; a[q][k] = s * pk + c * qk;
      }
    }
  }
  int o[3] = {0, 1, 2};                                                   // descending, stable
  for (int i = 1; i < 3; ++i)
    for (int j = i; j > 0 && a[o[j]][o[j]] > a[o[j - 1]][o[j - 1]]; --j) { const int t = o[j]; o[j] = o[j - 1]; o[j - 1] = t; }
  double e[3][3];                                                         // e[k] = axis k
  for (int k = 0; k < 2; ++k) {
    int big = 0;
    for (int r = 1; r < 3; ++r) if (fabs(v[r][o[k]]) > fabs(v[big][o[k]])) big = r;
    const double sg = v[big][o[k]] < 0.0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r) e[k][r] = sg * v[r][o[k]];
  }
  e[2][0] = e[0][1] * e[1][2] - e[0][2] * e[1][1];
  e[2][1] = e[0][2] * e[1][0] - e[0][0] * e[1][2];
  e[2][2] = e[0][0] * e[1][1] - e[0][1] * e[1][0];
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r) dbl[kDAxes + 3 * k + r] = e[k][r];
}

// One thread per row.  proj.w = 1 for a kept row (getLength <= max_distance: float products and sums, float sqrt, widened), else 0.
__global__ __launch_bounds__(kMThreads) void m2dp_project(const float4* __restrict__ pts, int n, const double* __restrict__ dbl, double max_distance,
                                                          float4* __restrict__ proj, int32_t* __restrict__ ctl) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kMThreads + threadIdx.x;
  bool kept = false;
  if (i < n) {
    const float4 p = pts[i];
    const double x = (double)p.x - dbl[kDMean], y = (double)p.y - dbl[kDMean + 1], z = (double)p.z - dbl[kDMean + 2];
    const double* e = dbl + kDAxes;
    const float a = (float)((e[0] * x + e[1] * y) + e[2] * z), b = (float)((e[3] * x + e[4] * y) + e[5] * z),
                c = (float)((e[6] * x + e[7] * y) + e[8] * z);
    const float len = sqrtf((a * a + b * b) + c * c);
    kept = (double)len <= max_distance;                                  // false for a NaN
    proj[i] = make_float4(a, b, c, kept ? 1.f : 0.f);
  }
  const unsigned long long m = __ballot(kept);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ctl[1], __popcll(m));
}

// views: six floats per view, projected_x_axis then projected_y_axis (made on the host as :74-82 make them).  blockIdx.y selects
// the slice of `vs` views this workgroup counts; its LDS holds vs x L x TB counters, TB = the reachable angular bins.  The view
// loop's loads have a wave-uniform address (scalar loads); a point's coordinates stay in registers for all views.
__global__ __launch_bounds__(kMHistThreads) void m2dp_hist(const float4* __restrict__ proj, int n, const float* __restrict__ views, int n_views,
                                                          int vs, int L, int T, int TB, double r, double angle_step, int32_t* __restrict__ A) {
#pragma clang fp contract(off)
  extern __shared__ int32_t s_cnt[];
  const int v0 = blockIdx.y * vs, nv = min(vs, n_views - v0), cells = nv * L * TB;
  for (int c = threadIdx.x; c < cells; c += kMHistThreads) s_cnt[c] = 0;
  __syncthreads();
  for (int i = blockIdx.x * kMHistThreads + threadIdx.x; i < n; i += gridDim.x * kMHistThreads) {
    const float4 p = proj[i];
    if (p.w == 0.f) continue;
    for (int v = 0; v < nv; ++v) {
      const float* ax = views + 6 * (v0 + v);
      const float a = fabsf(p.x * ax[0] + (p.y * ax[1] + p.z * ax[2]));  // (p^T axis).norm(): Eigen's x0 y0 + (x1 y1 + x2 y2)
      const float b = fabsf(p.x * ax[3] + (p.y * ax[4] + p.z * ax[5]));
      const float len = sqrtf(a * a + b * b);                            // Vector2f::norm
      const float ang = atan2f(b, a);                                    // a, b >= 0: never negative
      int li = (int)floor(sqrt((double)len / r));                        // :104
      int ti = (int)floor((double)ang / angle_step);                     // :109
      li = max(0, min(li, L - 1));                                       // :106-108
      // :110-112, and the bound of the LDS index: TB - 1 = min(t/4, t - 1).  A sample lands above t/4 only if atan2f of two
      // non-negative arguments exceeded float(pi/2); OCML's does not.  If it ever did, the sample would be folded into bin
      // t/4 here without a signal (the row sums of A would not show it).
      ti = max(0, min(ti, TB - 1));
      atomicAdd(&s_cnt[(v * L + li) * TB + ti], 1);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cells; c += kMHistThreads) {
    const int cnt = s_cnt[c];
    if (cnt == 0) continue;
    const int ti = c % TB, li = (c / TB) % L, v = c / (TB * L);
    atomicAdd(&A[(size_t)(v0 + v) * L * T + li * T + ti], cnt);
  }
}

// G = A A^T: workgroup i holds row i in LDS, its waves take the rows j in turn; int64 sums (exact, order-free), stored as f64
__global__ __launch_bounds__(kMThreads) void m2dp_gram(const int32_t* __restrict__ A, int n_views, int cols, double* __restrict__ dbl) {
  extern __shared__ int32_t s_row[];
  const int i = blockIdx.x;
  for (int c = threadIdx.x; c < cols; c += kMThreads) s_row[c] = A[(size_t)i * cols + c];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int j = threadIdx.x >> 6; j < n_views; j += kMThreads / 64) {
    long long acc = 0;
    for (int c = lane; c < cols; c += 64) acc += (long long)s_row[c] * (long long)A[(size_t)j * cols + c];
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
    if (lane == 0) dbl[kDG + i * n_views + j] = (double)acc;
  }
}

// One workgroup.  Cyclic Jacobi on G (nv x nv, f64, in LDS) in the round-robin order: a step rotates nv/2 disjoint pairs, which
// commute with one another, so the sweep equals a sequential one in that order.  The eigenvectors accumulate in dbl[kDV].  Then
// u1 = the eigenvector of the largest eigenvalue, v1 = A^T u1 / sigma1, both negated when sum(u1) < 0; desc = u1, v1 as float.
__global__ __launch_bounds__(kMDescThreads) void m2dp_descriptor(const int32_t* __restrict__ A, int nv, int cols, double* __restrict__ dbl,
                                                                float* __restrict__ desc, int32_t* __restrict__ ctl) {
  __shared__ double S[kMMaxViews * kMMaxViews];
  __shared__ double s_c[kMMaxViews / 2], s_s[kMMaxViews / 2], s_u[kMMaxViews];
  __shared__ int s_p[kMMaxViews / 2], s_q[kMMaxViews / 2];
  __shared__ int s_rot, s_top;
  __shared__ double s_sigma, s_tol;
  double* V = dbl + kDV;
  const int tid = threadIdx.x;
  for (int e = tid; e < nv * nv; e += kMDescThreads) { S[e] = dbl[kDG + e]; V[e] = (e / nv == e % nv) ? 1.0 : 0.0; }
  __syncthreads();
  if (tid == 0) {
    double big = 0.0;
    for (int k = 0; k < nv; ++k) big = fmax(big, fabs(S[k * nv + k]));
    s_tol = 1.0e-15 * big;                                              // off-diagonal entries below this are left alone
  }
  const int m = nv + (nv & 1), half = m / 2;                             // an odd size plays against an idle index
  int sweep = 0;
  for (; sweep < kMMaxSweeps; ++sweep) {
    if (tid == 0) s_rot = 0;
    __syncthreads();
    for (int step = 0; step < m - 1; ++step) {
      if (tid < half) {
        const int a = tid == 0 ? m - 1 : (step + tid) % (m - 1), b = tid == 0 ? step : (step - tid + (m - 1)) % (m - 1);
        const int p = min(a, b), q = max(a, b);
        double c = 1.0, s = 0.0;
        if (q < nv) {
          const double apq = S[p * nv + q];
          if (fabs(apq) > s_tol) { m2dp_rotation(S[p * nv + p], S[q * nv + q], apq, c, s); s_rot = 1; }
        }
        s_p[tid] = p; s_q[tid] = q; s_c[tid] = c; s_s[tid] = s;
      }
      __syncthreads();
      for (int it = tid; it < nv * half; it += kMDescThreads) {          // columns p, q of S and of V
        const int k = it / half, pr = it % half;
        const double s = s_s[pr];
        if (s == 0.0) continue;
        const double c = s_c[pr];
        const int p = s_p[pr], q = s_q[pr];
        const double kp = S[k * nv + p], kq = S[k * nv + q];
        S[k * nv + p] = c * kp - s * kq; S[k * nv + q] = s * kp + c * kq;
        const double vp = V[k * nv + p], vq = V[k * nv + q];
        V[k * nv + p] = c * vp - s * vq; V[k * nv + q] = s * vp + c * vq;
      }
      __syncthreads();
      for (int it = tid; it < nv * half; it += kMDescThreads) {          // rows p, q of S
        const int k = it / half, pr = it % half;
        const double s = s_s[pr];
        if (s == 0.0) continue;
        const double c = s_c[pr];
        const int p = s_p[pr], q = s_q[pr];
        const double pk = S[p * nv + k], qk = S[q * nv + k];
        S[p * nv + k] = c * pk - s * qk; S[q * nv + k] = s * pk + c * qk;
      }
      __syncthreads();
    }
    if (s_rot == 0) break;                                               // (read after the step's last barrier; written after the next one)
    __syncthreads();
  }
  if (tid == 0) {
    int top = 0;
    for (int k = 1; k < nv; ++k) if (S[k * nv + k] > S[top * nv + top]) top = k;
    const double lam = S[top * nv + top];
    double sum = 0.0;
    for (int k = 0; k < nv; ++k) sum += V[k * nv + top];
    s_top = top;
    s_sigma = lam > 0.0 ? (sum < 0.0 ? -sqrt(lam) : sqrt(lam)) : 0.0;    // the sign rides on sigma
    ctl[2] = lam > 0.0 ? 0 : 1;
    ctl[3] = sweep;
  }
  __syncthreads();
  if (s_sigma == 0.0) return;
  const double sg = s_sigma < 0.0 ? -1.0 : 1.0, sigma = fabs(s_sigma);
  if (tid < nv) { const double u = sg * V[tid * nv + s_top]; s_u[tid] = u; desc[tid] = (float)u; }
  __syncthreads();
  for (int c = tid; c < cols; c += kMDescThreads) {
    double acc = 0.0;
    for (int k = 0; k < nv; ++k) acc += (double)A[(size_t)k * cols + c] * s_u[k];
    desc[nv + c] = (float)(acc / sigma);
  }
}

}  // namespace

// what a handle keeps for the descriptor: allocated at the limits on first use, nothing afterwards
struct smhip_m2dp_state {
  float4* proj = nullptr;
  double* dbl = nullptr;
  int32_t* A = nullptr;
  float* views = nullptr;
  int32_t* ctl = nullptr;
  float* desc = nullptr;
  float* pinned = nullptr;          // views (6 x kMMaxViews), then the descriptor, then the ctl words
  smhip_m2dp_options opts{};        // of the views resident on the device
  bool have_views = false;
  int last_n = -1, last_views = 0, last_cols = 0;      // what smhip_m2dp_last can return (-1: nothing)
};

namespace {

constexpr int kPinViews = 0, kPinDesc = 6 * kMMaxViews, kPinCtl = kPinDesc + kMMaxViews + kMMaxCols, kPinTotal = kPinCtl + kCtl;

// nullptr = the options can run; *L = the ring count
const char* m2dp_problem(const smhip_m2dp_options* o, int* L) {
  if (!o) return "null options";
  if (!std::isfinite(o->r) || !std::isfinite(o->max_distance)) return "r and max_distance must be finite";
  if (o->r < 1.e-6) return "r is too small (m2dp.cc:64)";
  if (!(o->max_distance > 0.0)) return "max_distance must be positive";
  if (o->t < 1 || o->p < 1 || o->q < 1) return "t, p and q must be at least 1";
  if ((long long)o->p * o->q > kMMaxViews) return "p * q above the device limit of 64 views";
  const double l = std::ceil(std::sqrt(o->max_distance / o->r));          // :68
  if (!(l >= 1.0) || l * (double)o->t > (double)kMMaxCols) return "ceil(sqrt(max_distance / r)) * t above the device limit of 8192 columns";
  *L = (int)l;
  return nullptr;
}

smhip_status m2dp_ensure(smhip_context* h) {
  if (h->m2dp) return SMHIP_OK;
  auto* st = new smhip_m2dp_state;
  const int cap = std::max(h->dev.ns_cap, h->dev.nt_cap);
  smhip_status s = dev_alloc(h, &st->proj, (size_t)cap);
  if (!s) s = dev_alloc(h, &st->dbl, (size_t)kDTotal);
  if (!s) s = dev_alloc(h, &st->A, (size_t)kMMaxViews * kMMaxCols);
  if (!s) s = dev_alloc(h, &st->views, (size_t)6 * kMMaxViews);
  if (!s) s = dev_alloc(h, &st->ctl, (size_t)kCtl);
  if (!s) s = dev_alloc(h, &st->desc, (size_t)kMMaxViews + kMMaxCols);
  if (!s && hipHostMalloc(reinterpret_cast<void**>(&st->pinned), sizeof(float) * kPinTotal) != hipSuccess) { h->err = "m2dp: pinned allocation failed"; s = SMHIP_ERR_HIP; }
  if (s) { delete st; return s; }                                        // (device arrays stay with the handle's allocations)
  h->m2dp = st;
  return SMHIP_OK;
}

// projected_x_axis and projected_y_axis of every view, m2dp.cc:74-82, in float as Eigen evaluates them
void m2dp_views(const smhip_m2dp_options& o, float* out) {
#pragma clang fp contract(off)
  const double theta_step = M_PI / o.p, phi_step = M_PI_2 / o.q;          // :132-133
  for (int p = 0; p < o.p; ++p)
    for (int q = 0; q < o.q; ++q) {
      const double theta = p * theta_step, phi = q * phi_step;
      const float m[3] = {(float)(std::cos(theta) * std::cos(phi)), (float)(std::cos(theta) * std::sin(phi)), (float)std::sin(theta)};
      const float a = std::fabs(m[0]);                                    // (e1^T m).norm()
      const float am[3] = {a * m[0], a * m[1], a * m[2]};
      const float x[3] = {1.f - am[0], 0.f - am[1], 0.f - am[2]};
      const float c0a = m[1] * x[2], c0b = m[2] * x[1], c1a = m[2] * x[0], c1b = m[0] * x[2], c2a = m[0] * x[1], c2b = m[1] * x[0];
      float* w = out + 6 * (p * o.q + q);
      w[0] = x[0]; w[1] = x[1]; w[2] = x[2];
      w[3] = c0a - c0b; w[4] = c1a - c1b; w[5] = c2a - c2b;
    }
}

smhip_status m2dp_run(smhip_context* h, const float4* pts, int n, const smhip_m2dp_options& o, int L, float* descriptor) {
  smhip_m2dp_state* st = h->m2dp;
  hipStream_t s = h->stream;
  const int nv = o.p * o.q, cols = L * o.t, TB = std::min(o.t / 4, o.t - 1) + 1;
  if (!st->have_views || std::memcmp(&st->opts, &o, sizeof(o)) != 0) {
    m2dp_views(o, st->pinned + kPinViews);
    HIPCHK(h, hipMemcpyAsync(st->views, st->pinned + kPinViews, sizeof(float) * 6 * nv, hipMemcpyHostToDevice, s));
    st->opts = o; st->have_views = true;
  }
  st->last_n = -1;
  HIPCHK(h, hipMemsetAsync(st->A, 0, sizeof(int32_t) * (size_t)nv * cols, s));
  HIPCHK(h, hipMemsetAsync(st->ctl, 0, sizeof(int32_t) * kCtl, s));
  const int parts = std::min(kMParts, (n + kMThreads - 1) / kMThreads), rows = (n + kMThreads - 1) / kMThreads;
  hipLaunchKernelGGL(m2dp_sums, dim3(parts), dim3(kMThreads), 0, s, pts, n, st->dbl, st->ctl);
  hipLaunchKernelGGL(m2dp_mean, dim3(1), dim3(64), 0, s, parts, n, st->dbl);
  hipLaunchKernelGGL(m2dp_cov, dim3(parts), dim3(kMThreads), 0, s, pts, n, st->dbl);
  hipLaunchKernelGGL(m2dp_axes, dim3(1), dim3(64), 0, s, parts, n, st->dbl);
  hipLaunchKernelGGL(m2dp_project, dim3(rows), dim3(kMThreads), 0, s, pts, n, st->dbl, o.max_distance, st->proj, st->ctl);
  const int per_view = L * TB;                                            // <= kMMaxCols counters: one view always fits
  const int vs = std::max(1, std::min(nv, kMSliceCells / per_view)), slices = (nv + vs - 1) / vs;
  const int hb = std::min(kMHistBlocks, (n + kMHistThreads - 1) / kMHistThreads);
  hipLaunchKernelGGL(m2dp_hist, dim3(hb, slices), dim3(kMHistThreads), sizeof(int32_t) * (size_t)vs * per_view, s, st->proj, n, st->views, nv, vs, L,
                     o.t, TB, o.r, 2.0 * M_PI / o.t, st->A);
  hipLaunchKernelGGL(m2dp_gram, dim3(nv), dim3(kMThreads), sizeof(int32_t) * (size_t)cols, s, st->A, nv, cols, st->dbl);
  hipLaunchKernelGGL(m2dp_descriptor, dim3(1), dim3(kMDescThreads), 0, s, st->A, nv, cols, st->dbl, st->desc, st->ctl);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(st->pinned + kPinDesc, st->desc, sizeof(float) * (nv + cols), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(st->pinned + kPinCtl, st->ctl, sizeof(int32_t) * kCtl, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  int32_t ctl[kCtl];
  std::memcpy(ctl, st->pinned + kPinCtl, sizeof(ctl));
  if (ctl[0]) { h->err = "m2dp: a row has a non-finite coordinate"; return SMHIP_ERR_INVALID_ARGUMENT; }
  st->last_n = n; st->last_views = nv; st->last_cols = cols;
  if (ctl[2]) { h->err = "m2dp: no row lies within max_distance of the centroid (sigma1 = 0)"; return SMHIP_ERR_INVALID_ARGUMENT; }
  std::memcpy(descriptor, st->pinned + kPinDesc, sizeof(float) * (nv + cols));
  return SMHIP_OK;
}

}  // namespace

extern "C" {

void smhip_internal_free_m2dp(smhip_context* h) {
  if (!h->m2dp) return;
  if (h->m2dp->pinned) (void)hipHostFree(h->m2dp->pinned);
  delete h->m2dp;
  h->m2dp = nullptr;
}

void smhip_m2dp_default_options(smhip_m2dp_options* o) {
  if (!o) return;
  o->r = 0.1; o->max_distance = 100.; o->t = 16; o->p = 4; o->q = 16;     // m2dp.h:48-49
}

int smhip_m2dp_length(const smhip_m2dp_options* o) {
  int L = 0;
  if (m2dp_problem(o, &L)) return -1;
  return o->p * o->q + L * o->t;
}

smhip_status smhip_m2dp_f32(smhip_handle h, const float* points, int stride_floats, int n, const smhip_m2dp_options* opts, float* descriptor, int len) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  int L = 0;
  if (!points || !descriptor || (stride_floats != 4 && stride_floats != 5)) {
    h->err = "m2dp: bad arguments (null pointer, or a stride other than 4 = x y z intensity or 5 = InnerPointType)";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  if (const char* why = m2dp_problem(opts, &L)) { h->err = std::string("m2dp: ") + why; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (n < 2) { h->err = "m2dp: at least two rows are needed (the covariance divides by n - 1)"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (len != opts->p * opts->q + L * opts->t) { h->err = "m2dp: len must equal smhip_m2dp_length(opts)"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (n > std::max(h->dev.ns_cap, h->dev.nt_cap)) { h->err = "m2dp: cloud larger than the handle's capacity"; return SMHIP_ERR_CAPACITY; }
  HIPCHK(h, hipSetDevice(h->device));
  smhip_status s = prep_ensure(h);
  if (!s) s = m2dp_ensure(h);
  if (s) return s;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (stride_floats == 4) std::memcpy(h->stage, points, sizeof(float4) * (size_t)n);
  else for (int i = 0; i < n; ++i) { const float* r = points + 5 * (size_t)i; h->stage[i] = make_float4(r[0], r[1], r[2], r[3]); }
  HIPCHK(h, hipMemcpyAsync(h->prep_raw, h->stage, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  return m2dp_run(h, h->prep_raw, n, *opts, L, descriptor);
}

smhip_status smhip_m2dp_from_filter_output(smhip_handle h, const smhip_m2dp_options* opts, float* descriptor, int len) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  int L = 0;
  if (!descriptor) { h->err = "m2dp: null descriptor"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (const char* why = m2dp_problem(opts, &L)) { h->err = std::string("m2dp: ") + why; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (len != opts->p * opts->q + L * opts->t) { h->err = "m2dp: len must equal smhip_m2dp_length(opts)"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (!h->filt || filt_count(h->filt) <= 0) { h->err = "m2dp: no filtered or built cloud is resident"; return SMHIP_ERR_NOT_READY; }
  const int n = filt_count(h->filt);
  if (n < 2) { h->err = "m2dp: at least two rows are needed (the covariance divides by n - 1)"; return SMHIP_ERR_INVALID_ARGUMENT; }
  HIPCHK(h, hipSetDevice(h->device));
  const smhip_status s = m2dp_ensure(h);
  if (s) return s;
  return m2dp_run(h, filt_points(h->filt), n, *opts, L, descriptor);
}

smhip_status smhip_m2dp_last(smhip_handle h, float* projected3, int32_t* kept, int32_t* A, int a_len, int* n_kept) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  smhip_m2dp_state* st = h->m2dp;
  if (!st || st->last_n < 0) { h->err = "m2dp: no descriptor has been computed (or the last cloud had a non-finite row)"; return SMHIP_ERR_NOT_READY; }
  if (A && a_len != st->last_views * st->last_cols) { h->err = "m2dp: a_len must equal p * q * l * t of the last call"; return SMHIP_ERR_INVALID_ARGUMENT; }
  HIPCHK(h, hipSetDevice(h->device));
  const int n = st->last_n;
  std::vector<float4> p;
  if (projected3 || kept) {
    p.resize((size_t)n);
    HIPCHK(h, hipMemcpyAsync(p.data(), st->proj, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  }
  if (A) HIPCHK(h, hipMemcpyAsync(A, st->A, sizeof(int32_t) * (size_t)a_len, hipMemcpyDeviceToHost, h->stream));
  int32_t ctl[kCtl] = {0, 0, 0, 0};
  HIPCHK(h, hipMemcpyAsync(ctl, st->ctl, sizeof(ctl), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < p.size(); ++i) {
    if (projected3) { projected3[3 * i] = p[i].x; projected3[3 * i + 1] = p[i].y; projected3[3 * i + 2] = p[i].z; }
    if (kept) kept[i] = p[i].w != 0.f ? 1 : 0;
  }
  if (n_kept) *n_kept = ctl[1];
  return SMHIP_OK;
}

double smhip_m2dp_match(const float* P, const float* Q, int n) {
  if (!P || !Q || n < 10) return -1.;                                     // m2dp.cc:153-156
  double pq = 0, pp = 0, qq = 0, sp = 0, sq = 0;
  for (int i = 0; i < n; ++i) {
    const double a = P[i], b = Q[i];
    pq += a * b; pp += a * a; qq += b * b; sp += a; sq += b;
  }
  const double N = n;
  return std::fabs((N * pq - sp * sq) / std::sqrt((N * pp - sp * sp) * (N * qq - sq * sq)));   // :162-168
}

}  // extern "C"
