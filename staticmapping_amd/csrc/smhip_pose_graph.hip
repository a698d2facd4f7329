// smhip_pose_graph.hip -- the pose-graph optimiser (what back_end::IsamOptimizer asks of GTSAM, back_end/isam_optimizer.{h,cc}) on
// the device: the kernel and the C ABI.  The definition is DESIGN.md section 6 ("Pose graph"), restated in tests/pose_graph_ref.py.
//
// One optimisation is ONE launch of pose_graph_solve: one workgroup of 1024 threads runs every Gauss-Newton step, every
// conjugate-gradient iteration and every level of the preconditioner's cyclic reduction, with __syncthreads as the only barrier
// and nothing read back in between (pose_graph_kernel.h holds the loop; it also compiles for a CPU).  The work between two
// barriers is a few thousand 6x6 block operations at most, so a grid-wide seam would cost more than what it separates.
//   linearise     one thread per factor: e, the whitened A and B; the only place that knows a factor's kind (BETWEEN, PRIOR, POINT,
//                 HANDEYE: include/smhip.h, "Factor kinds", "Odometry calibration factor") and, with the cost, its Huber threshold
//                 ("Robust factors")
//   assemble      one thread per node, its edges in index order (the host's CSR list): Hkk, g, the chain block -- no atomics
//   factor        block cyclic reduction of M = the block-tridiagonal part of H + lambda blockdiag(H): two barriers per level
//   pcg           H p matrix-free (per edge, then per node), M^-1 by one sweep up and one down the levels, dot products as
//                 per-thread partials folded by wave shuffles and then in wave order: two calls give the same bits
// The refusals and the CSR list are made on the host (pose_graph_plan.h) before anything is touched.
//
// smhip_pose_graph_marginals ("Marginal covariances") is two launches: pose_graph_solve with probe = 3 leaves the
// Gauss-Newton matrix of the last call's final poses and its preconditioner's factors in global memory, then pose_graph_marginals, one
// workgroup per CU at most, solves six columns per queried node against them -- many independent solves against one fixed matrix.
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "pose_graph_kernel.h"
#include "pose_graph_plan.h"
#include "smhip_context.h"

using namespace smhip_host;
namespace pg = smhip::pose_graph;

namespace {

constexpr int kPgThreads = 1024;

struct BlockCtx {
  double* part;                    // one slot per wave, in LDS
  __device__ int tid() const { return (int)threadIdx.x; }
  __device__ int nthreads() const { return kPgThreads; }
  __device__ void sync() const { __syncthreads(); }
  __device__ double sum(double v) const {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < kPgThreads / 64; ++w) t += part[w];
    __syncthreads();
    return t;
  }
  __device__ double max(double v) const {
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = part[0];
    for (int w = 1; w < kPgThreads / 64; ++w) t = fmax(t, part[w]);
    __syncthreads();
    return t;
  }
};

__global__ __launch_bounds__(kPgThreads) void pose_graph_solve(const pg::Dev d) {
  __shared__ double s_part[kPgThreads / 64];
  BlockCtx c{s_part};
  pg::run(d, c);
}

// Marginal covariances (pose_graph_kernel.h, "marginal covariances"): workgroup w takes queries w, w + G, w + 2G, ... and runs each
// one's six column solves through its own slice of ws.  `shared` is only read; no atomics, no grid barrier, nothing between workgroups.
__global__ __launch_bounds__(kPgThreads) void pose_graph_marginals(const pg::Dev shared, int n_query, const int32_t* query, int n_rows, const int32_t* rows,
                                                                   double* ws, size_t ws_stride, double* cov, double* blocks, int32_t* info) {
  __shared__ double s_part[kPgThreads / 64];
  BlockCtx c{s_part};
  pg::Dev d = shared;
  pg::marginal_slice(&d, ws + ws_stride * (size_t)blockIdx.x);
  pg::marginal_queries(d, c, (int)blockIdx.x, (int)gridDim.x, n_query, query, n_rows, rows, cov, blocks, info);
}

// doubles and words of the device state per node / per edge, and of the staging the host fills
constexpr int kNodeD = 3 * 12 + 7 * 36 + 7 * 6 + 2 * 6, kEdgeD = 12 + 6 + 2 * 36 + 2 * 6 + 4 + 36;      // (+ huber, wgt, rep_s, rep_c; sqrt_info)
constexpr int kNodeI = 2, kEdgeI = 6;           // fixed, csr_off (+1); ij, csr_edge, kind, info_index

}  // namespace

struct smhip_pose_graph_state {
  double* dbl = nullptr;           // device
  int32_t* ints = nullptr;
  pg::Dev dev{};
  std::vector<double> host_d;      // staging, sized once
  std::vector<int32_t> host_i;
  pg::Plan plan;
  int last_n = -1, last_m = 0;     // what smhip_pose_graph_last can run again (-1: nothing)
  bool last_huber = false;         // that call uploaded thresholds
  bool last_info = false;          // ... and square-root informations
  bool last_numeric = false;       // ... and ended NUMERIC: cur is no result (smhip_pose_graph_marginals answers NOT_READY)
  // smhip_pose_graph_marginals' own: grown to fit a call, never shrunk, freed with the state
  double *marg_ws = nullptr, *marg_out = nullptr;      // the workgroups' slices; cov then blocks
  int32_t* marg_int = nullptr;                         // query, rows, info
  size_t marg_ws_cap = 0, marg_out_cap = 0, marg_int_cap = 0;      // in elements
  int cus = 0;                                         // the device's CU count (0: not asked yet)
  std::vector<double> marg_host_d;
  std::vector<int32_t> marg_host_i;
};

namespace {

smhip_status pg_ensure(smhip_context* h) {
  if (h->pose_graph) return SMHIP_OK;
  auto* st = new smhip_pose_graph_state;
  const size_t N = pg::kMaxNodes, M = pg::kMaxEdges;
  const size_t nd = N * kNodeD + M * kEdgeD + pg::kOutDoubles, ni = N * kNodeI + 1 + M * kEdgeI + pg::kOutInts;
  smhip_status s = dev_alloc(h, &st->dbl, nd);
  if (!s) s = dev_alloc(h, &st->ints, ni);
  if (s) { delete st; return s; }
  double* p = st->dbl;
  auto take = [&p](size_t count) { double* r = p; p += count; return r; };
  pg::Dev& d = st->dev;
  // (what the host uploads: pose0, Z, sinv, huber; v for the probe)
  d.pose0 = take(12 * N); d.Z = take(12 * M); d.sinv = take(6 * M); d.huber = take(M);
  d.v = take(6 * N); d.minv = take(6 * N);
  d.cur = take(12 * N); d.cand = take(12 * N);
  d.Hkk = take(36 * N); d.C = take(36 * N); d.D = take(36 * N); d.U = take(36 * N); d.Dinv = take(36 * N); d.Wm = take(36 * N); d.Wp = take(36 * N);
  d.g = take(6 * N); d.x = take(6 * N); d.r = take(6 * N); d.z = take(6 * N); d.p = take(6 * N); d.q = take(6 * N); d.b = take(6 * N);
  d.A = take(36 * M); d.B = take(36 * M); d.rw = take(6 * M); d.u = take(6 * M);
  d.wgt = take(M); d.rep_s = take(M); d.rep_c = take(M);
  d.sqrt_info = take(36 * M);
  d.out_d = take(pg::kOutDoubles);
  int32_t* q = st->ints;
  auto takei = [&q](size_t count) { int32_t* r = q; q += count; return r; };
  // (uploaded: fixed, csr_off, ij, csr_edge, kind)
  d.fixed = takei(N); d.csr_off = takei(N + 1); d.ij = takei(2 * M); d.csr_edge = takei(2 * M); d.kind = takei(M);
  d.info_index = takei(M);
  d.out_i = takei(pg::kOutInts);
  st->host_d.resize(12 * N + 12 * M + 6 * M);
  st->host_i.resize(N + (N + 1) + 2 * M + 2 * M + M);
  h->pose_graph = st;
  return SMHIP_OK;
}

// column-major 4x4 -> 12 doubles, the rotation row-major then the translation
void pack12(const double* m, double* o) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) o[3 * r + c] = m[4 * c + r];
    o[9 + r] = m[12 + r];
  }
}

smhip_status pg_plan(bool calib, int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds, const int32_t* ij, const double* data,
                     const double* sigmas, const double* huber, int32_t* csr_offsets, int32_t* csr_edges, char* why, int why_len,
                     bool info = false, const int32_t* info_index = nullptr, const double* sqrt_info = nullptr) {
  pg::Plan plan;
  std::string text;
  const smhip_status s = info ? pg::check_and_plan_info(n_nodes, poses, fixed, n_factors, kinds, ij, data, sigmas, huber, info_index, sqrt_info, &plan, nullptr, &text)
                              : pg::check_and_plan_calib(calib, n_nodes, poses, fixed, n_factors, kinds, ij, data, sigmas, huber, &plan, &text);
  if (why && why_len > 0) { std::strncpy(why, text.c_str(), (size_t)why_len - 1); why[why_len - 1] = '\0'; }
  if (s) return s;
  if (csr_offsets) std::memcpy(csr_offsets, plan.csr_offsets.data(), sizeof(int32_t) * plan.csr_offsets.size());
  if (csr_edges && !plan.csr_edges.empty()) std::memcpy(csr_edges, plan.csr_edges.data(), sizeof(int32_t) * plan.csr_edges.size());
  return SMHIP_OK;
}

// every optimise entry; calib: HANDEYE factors are accepted (smhip_pose_graph_optimize_calib); info: the *_info entry, whose BETWEEN
// factors may carry a 6x6 square-root information (a call in which none does uploads nothing more and launches what *_calib launches)
smhip_status pg_optimize(bool calib, smhip_handle h, int n_nodes, double* poses_inout, const uint8_t* fixed, int n_edges, const uint8_t* kinds,
                         const int32_t* edge_ij, const double* edge_Z, const double* edge_sigmas, const double* huber,
                         const smhip_pose_graph_options* opts, smhip_pose_graph_stats* stats,
                         bool info = false, const int32_t* info_index = nullptr, const double* sqrt_info = nullptr) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  smhip_pose_graph_options o;
  smhip_pose_graph_default_options(&o);
  if (opts) o = *opts;
  if (o.max_iterations < 1) { h->err = "pose graph: max_iterations must be at least 1"; return SMHIP_ERR_INVALID_ARGUMENT; }
  pg::Plan plan;
  int n_info = 0;
  if (info) {
    if (const smhip_status s = pg::check_and_plan_info(n_nodes, poses_inout, fixed, n_edges, kinds, edge_ij, edge_Z, edge_sigmas, huber, info_index, sqrt_info, &plan, &n_info, &h->err)) return s;
  } else if (const smhip_status s = pg::check_and_plan_calib(calib, n_nodes, poses_inout, fixed, n_edges, kinds, edge_ij, edge_Z, edge_sigmas, huber, &plan, &h->err)) {
    return s;
  }
  HIPCHK(h, hipSetDevice(h->device));
  if (const smhip_status s = pg_ensure(h)) return s;
  smhip_pose_graph_state* st = h->pose_graph;
  st->last_n = -1;
  st->plan = plan;
  const size_t N = pg::kMaxNodes, M = pg::kMaxEdges;
  double* hd = st->host_d.data();
  for (int k = 0; k < n_nodes; ++k) pack12(poses_inout + 16 * (size_t)k, hd + 12 * (size_t)k);
  int32_t* hi = st->host_i.data();
  const size_t n_csr = plan.csr_edges.size();
  for (int e = 0; e < n_edges; ++e) {
    const int kind = kinds ? kinds[e] : SMHIP_POSE_GRAPH_FACTOR_BETWEEN;
    double* z = hd + 12 * N + 12 * (size_t)e;
    double* sinv = hd + 12 * N + 12 * M + 6 * (size_t)e;
    hi[N + N + 1 + 4 * M + (size_t)e] = kind;
    if (kind == SMHIP_POSE_GRAPH_FACTOR_POINT) {                 // the lever arm, the point; three sigmas
      for (int c = 0; c < 12; ++c) z[c] = c < 6 ? edge_Z[16 * (size_t)e + c] : 0.0;
      for (int c = 0; c < 6; ++c) sinv[c] = c < 3 ? 1.0 / edge_sigmas[6 * (size_t)e + c] : 0.0;
      continue;
    }
    pack12(edge_Z + 16 * (size_t)e, z);
    for (int c = 0; c < 6; ++c) sinv[c] = 1.0 / (edge_sigmas ? edge_sigmas[6 * (size_t)e + c] : pg::kDefaultSigmas[c]);
  }
  for (int k = 0; k < n_nodes; ++k) hi[k] = fixed[k] ? 1 : 0;
  std::memcpy(hi + N, plan.csr_offsets.data(), sizeof(int32_t) * ((size_t)n_nodes + 1));
  if (n_edges > 0) {
    std::memcpy(hi + N + N + 1, edge_ij, sizeof(int32_t) * 2 * (size_t)n_edges);
    std::memcpy(hi + N + N + 1 + 2 * M, plan.csr_edges.data(), sizeof(int32_t) * n_csr);
  }
  hipStream_t s = h->stream;
  pg::Dev d = st->dev;
  d.n = n_nodes; d.m = n_edges; d.max_it = o.max_iterations; d.pcg_cap = plan.pcg_cap; d.pcg_budget = SMHIP_POSE_GRAPH_MAX_PCG_TOTAL; d.probe = 0;
  const bool robust = huber != nullptr && n_edges > 0;
  if (robust) HIPCHK(h, hipMemcpyAsync(const_cast<double*>(d.huber), huber, sizeof(double) * (size_t)n_edges, hipMemcpyHostToDevice, s));
  else d.huber = nullptr;
  const bool with_info = n_info > 0;
  if (with_info) {
    HIPCHK(h, hipMemcpyAsync(const_cast<int32_t*>(d.info_index), info_index, sizeof(int32_t) * (size_t)n_edges, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(const_cast<double*>(d.sqrt_info), sqrt_info, sizeof(double) * 36 * (size_t)n_info, hipMemcpyHostToDevice, s));
  } else {
    d.info_index = nullptr; d.sqrt_info = nullptr;
  }
  HIPCHK(h, hipMemcpyAsync(const_cast<double*>(d.pose0), hd, sizeof(double) * 12 * (size_t)n_nodes, hipMemcpyHostToDevice, s));
  if (n_edges > 0) {
    HIPCHK(h, hipMemcpyAsync(const_cast<double*>(d.Z), hd + 12 * N, sizeof(double) * 12 * (size_t)n_edges, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(const_cast<double*>(d.sinv), hd + 12 * N + 12 * M, sizeof(double) * 6 * (size_t)n_edges, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(const_cast<int32_t*>(d.ij), hi + N + N + 1, sizeof(int32_t) * 2 * (size_t)n_edges, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(const_cast<int32_t*>(d.csr_edge), hi + N + N + 1 + 2 * M, sizeof(int32_t) * n_csr, hipMemcpyHostToDevice, s));
    HIPCHK(h, hipMemcpyAsync(const_cast<int32_t*>(d.kind), hi + N + N + 1 + 4 * M, sizeof(int32_t) * (size_t)n_edges, hipMemcpyHostToDevice, s));
  }
  HIPCHK(h, hipMemcpyAsync(const_cast<int32_t*>(d.fixed), hi, sizeof(int32_t) * (size_t)n_nodes, hipMemcpyHostToDevice, s));
  HIPCHK(h, hipMemcpyAsync(const_cast<int32_t*>(d.csr_off), hi + N, sizeof(int32_t) * ((size_t)n_nodes + 1), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(pose_graph_solve, dim3(1), dim3(kPgThreads), 0, s, d);
  HIPCHK(h, hipGetLastError());
  double out_d[pg::kOutDoubles];
  int32_t out_i[pg::kOutInts];
  HIPCHK(h, hipMemcpyAsync(hd, d.cur, sizeof(double) * 12 * (size_t)n_nodes, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(out_d, d.out_d, sizeof(out_d), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(out_i, d.out_i, sizeof(out_i), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  st->last_n = n_nodes; st->last_m = n_edges; st->last_huber = robust; st->last_info = with_info;
  st->last_numeric = out_i[pg::kOutStop] == SMHIP_POSE_GRAPH_STOP_NUMERIC;
  if (stats) {
    stats->initial_cost = out_d[pg::kOutInitial]; stats->final_cost = out_d[pg::kOutFinal]; stats->damping = out_d[pg::kOutLambda];
    stats->stop_reason = out_i[pg::kOutStop]; stats->iterations = out_i[pg::kOutIterations];
    stats->accepted_steps = out_i[pg::kOutAccepted]; stats->rejected_steps = out_i[pg::kOutRejected];
    stats->pcg_iterations = out_i[pg::kOutPcg]; stats->pcg_max_iterations = out_i[pg::kOutPcgMax];
    stats->pcg_cap = plan.pcg_cap; stats->levels = plan.levels;
  }
  if (out_i[pg::kOutStop] == SMHIP_POSE_GRAPH_STOP_NUMERIC) {
    h->err = "pose graph: a pivot of the preconditioner's factorisation was not positive, or a sum was not finite; the poses are left as given";
    return SMHIP_ERR_NO_MATCH;
  }
  for (int k = 0; k < n_nodes; ++k) {
    if (fixed[k]) continue;
    const double* p = hd + 12 * (size_t)k;
    double* m = poses_inout + 16 * (size_t)k;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) m[4 * c + r] = p[3 * r + c];
      m[12 + r] = p[9 + r];
      m[4 * r + 3] = 0.0;
    }
    m[15] = 1.0;
  }
  return SMHIP_OK;
}

}  // namespace

extern "C" {

void smhip_internal_free_pose_graph(smhip_context* h) {
  if (smhip_pose_graph_state* st = h->pose_graph) {
    (void)hipFree(st->marg_ws); (void)hipFree(st->marg_out); (void)hipFree(st->marg_int);      // (nullptr is fine)
  }
  delete h->pose_graph;            // (the other device arrays are among the handle's allocations)
  h->pose_graph = nullptr;
}

void smhip_pose_graph_default_options(smhip_pose_graph_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_iterations = 50;
}

smhip_status smhip_pose_graph_plan_factors(int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds, const int32_t* ij,
                                           const double* data, const double* sigmas, int32_t* csr_offsets, int32_t* csr_edges, char* why, int why_len) {
  return smhip_pose_graph_plan_robust(n_nodes, poses, fixed, n_factors, kinds, ij, data, sigmas, nullptr, csr_offsets, csr_edges, why, why_len);
}

smhip_status smhip_pose_graph_plan_robust(int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds, const int32_t* ij,
                                          const double* data, const double* sigmas, const double* huber, int32_t* csr_offsets, int32_t* csr_edges, char* why,
                                          int why_len) {
  return pg_plan(false, n_nodes, poses, fixed, n_factors, kinds, ij, data, sigmas, huber, csr_offsets, csr_edges, why, why_len);
}

smhip_status smhip_pose_graph_plan_calib(int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds, const int32_t* ij,
                                         const double* data, const double* sigmas, const double* huber, int32_t* csr_offsets, int32_t* csr_edges, char* why,
                                         int why_len) {
  return pg_plan(true, n_nodes, poses, fixed, n_factors, kinds, ij, data, sigmas, huber, csr_offsets, csr_edges, why, why_len);
}

smhip_status smhip_pose_graph_plan(int n_nodes, const double* poses, const uint8_t* fixed, int n_edges, const int32_t* edge_ij, const double* edge_Z,
                                   const double* edge_sigmas, int32_t* csr_offsets, int32_t* csr_edges, char* why, int why_len) {
  return smhip_pose_graph_plan_factors(n_nodes, poses, fixed, n_edges, nullptr, edge_ij, edge_Z, edge_sigmas, csr_offsets, csr_edges, why, why_len);
}

smhip_status smhip_pose_graph_optimize(smhip_handle h, int n_nodes, double* poses_inout, const uint8_t* fixed, int n_edges, const int32_t* edge_ij,
                                       const double* edge_Z, const double* edge_sigmas, const smhip_pose_graph_options* opts,
                                       smhip_pose_graph_stats* stats) {
  return smhip_pose_graph_optimize_factors(h, n_nodes, poses_inout, fixed, n_edges, nullptr, edge_ij, edge_Z, edge_sigmas, opts, stats);
}

smhip_status smhip_pose_graph_optimize_factors(smhip_handle h, int n_nodes, double* poses_inout, const uint8_t* fixed, int n_edges, const uint8_t* kinds,
                                               const int32_t* edge_ij, const double* edge_Z, const double* edge_sigmas,
                                               const smhip_pose_graph_options* opts, smhip_pose_graph_stats* stats) {
  return smhip_pose_graph_optimize_robust(h, n_nodes, poses_inout, fixed, n_edges, kinds, edge_ij, edge_Z, edge_sigmas, nullptr, opts, stats);
}

smhip_status smhip_pose_graph_optimize_robust(smhip_handle h, int n_nodes, double* poses_inout, const uint8_t* fixed, int n_edges, const uint8_t* kinds,
                                              const int32_t* edge_ij, const double* edge_Z, const double* edge_sigmas, const double* huber,
                                              const smhip_pose_graph_options* opts, smhip_pose_graph_stats* stats) {
  return pg_optimize(false, h, n_nodes, poses_inout, fixed, n_edges, kinds, edge_ij, edge_Z, edge_sigmas, huber, opts, stats);
}

smhip_status smhip_pose_graph_optimize_calib(smhip_handle h, int n_nodes, double* poses_inout, const uint8_t* fixed, int n_edges, const uint8_t* kinds,
                                             const int32_t* edge_ij, const double* edge_Z, const double* edge_sigmas, const double* huber,
                                             const smhip_pose_graph_options* opts, smhip_pose_graph_stats* stats) {
  return pg_optimize(true, h, n_nodes, poses_inout, fixed, n_edges, kinds, edge_ij, edge_Z, edge_sigmas, huber, opts, stats);
}

smhip_status smhip_pose_graph_plan_info(int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds, const int32_t* ij,
                                        const double* data, const double* sigmas, const double* huber, const int32_t* info_index, const double* sqrt_info,
                                        int32_t* csr_offsets, int32_t* csr_edges, char* why, int why_len) {
  return pg_plan(true, n_nodes, poses, fixed, n_factors, kinds, ij, data, sigmas, huber, csr_offsets, csr_edges, why, why_len, true, info_index, sqrt_info);
}

smhip_status smhip_pose_graph_optimize_info(smhip_handle h, int n_nodes, double* poses_inout, const uint8_t* fixed, int n_edges, const uint8_t* kinds,
                                            const int32_t* edge_ij, const double* edge_Z, const double* edge_sigmas, const double* huber,
                                            const int32_t* info_index, const double* sqrt_info, const smhip_pose_graph_options* opts,
                                            smhip_pose_graph_stats* stats) {
  return pg_optimize(true, h, n_nodes, poses_inout, fixed, n_edges, kinds, edge_ij, edge_Z, edge_sigmas, huber, opts, stats, true, info_index, sqrt_info);
}

smhip_status smhip_pose_graph_last(smhip_handle h, int n_nodes, int n_edges, double* residuals, double* A, double* B, double* gradient, const double* v, double* minv_v) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  smhip_pose_graph_state* st = h->pose_graph;
  if (!st || st->last_n < 0) { h->err = "pose graph: no optimisation has been launched on this handle"; return SMHIP_ERR_NOT_READY; }
  if (n_nodes != st->last_n || n_edges != st->last_m) {
    h->err = "pose graph: the last optimisation had " + std::to_string(st->last_n) + " nodes and " + std::to_string(st->last_m) + " edges, not the sizes given";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  if (minv_v && !v) { h->err = "pose graph: minv_v needs v"; return SMHIP_ERR_INVALID_ARGUMENT; }
  HIPCHK(h, hipSetDevice(h->device));
  const int n = st->last_n, m = st->last_m;
  hipStream_t s = h->stream;
  pg::Dev d = st->dev;
  d.n = n; d.m = m; d.max_it = 0; d.pcg_cap = 0; d.probe = 1;
  if (!st->last_huber) d.huber = nullptr;
  if (!st->last_info) { d.info_index = nullptr; d.sqrt_info = nullptr; }
  if (v) HIPCHK(h, hipMemcpyAsync(const_cast<double*>(d.v), v, sizeof(double) * 6 * (size_t)n, hipMemcpyHostToDevice, s));
  else HIPCHK(h, hipMemsetAsync(const_cast<double*>(d.v), 0, sizeof(double) * 6 * (size_t)n, s));
  hipLaunchKernelGGL(pose_graph_solve, dim3(1), dim3(kPgThreads), 0, s, d);
  HIPCHK(h, hipGetLastError());
  if (residuals && m > 0) HIPCHK(h, hipMemcpyAsync(residuals, d.rw, sizeof(double) * 6 * (size_t)m, hipMemcpyDeviceToHost, s));
  if (A && m > 0) HIPCHK(h, hipMemcpyAsync(A, d.A, sizeof(double) * 36 * (size_t)m, hipMemcpyDeviceToHost, s));
  if (B && m > 0) HIPCHK(h, hipMemcpyAsync(B, d.B, sizeof(double) * 36 * (size_t)m, hipMemcpyDeviceToHost, s));
  if (gradient) HIPCHK(h, hipMemcpyAsync(gradient, d.g, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost, s));
  if (minv_v) HIPCHK(h, hipMemcpyAsync(minv_v, d.minv, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  return SMHIP_OK;
}

smhip_status smhip_pose_graph_last_robust(smhip_handle h, int n_factors, double* norm, double* weight, double* cost) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  smhip_pose_graph_state* st = h->pose_graph;
  if (!st || st->last_n < 0) { h->err = "pose graph: no optimisation has been launched on this handle"; return SMHIP_ERR_NOT_READY; }
  if (n_factors != st->last_m) {
    h->err = "pose graph: the last optimisation had " + std::to_string(st->last_m) + " factors, not the count given";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  HIPCHK(h, hipSetDevice(h->device));
  const int m = st->last_m;
  if (m == 0) return SMHIP_OK;
  hipStream_t s = h->stream;
  pg::Dev d = st->dev;
  d.n = st->last_n; d.m = m; d.max_it = 0; d.pcg_cap = 0; d.probe = 2;
  if (!st->last_huber) d.huber = nullptr;
  if (!st->last_info) { d.info_index = nullptr; d.sqrt_info = nullptr; }
  hipLaunchKernelGGL(pose_graph_solve, dim3(1), dim3(kPgThreads), 0, s, d);
  HIPCHK(h, hipGetLastError());
  if (norm) HIPCHK(h, hipMemcpyAsync(norm, d.rep_s, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, s));
  if (weight) HIPCHK(h, hipMemcpyAsync(weight, d.wgt, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, s));
  if (cost) HIPCHK(h, hipMemcpyAsync(cost, d.rep_c, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  return SMHIP_OK;
}

void smhip_pose_graph_marginals_default_options(smhip_pose_graph_marginals_options* o) {
  if (o) std::memset(o, 0, sizeof(*o));
}

smhip_status smhip_pose_graph_marginals(smhip_handle h, int n_nodes, int n_query, const int32_t* query, double* cov, int n_rows, const int32_t* rows,
                                        double* blocks, const smhip_pose_graph_marginals_options* opts, smhip_pose_graph_marginals_stats* stats) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  smhip_pose_graph_state* st = h->pose_graph;
  if (st && st->last_n >= 0 && !st->cus) {
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipDeviceGetAttribute(&st->cus, hipDeviceAttributeMultiprocessorCount, h->device));
  }
  int G = 0;
  if (const smhip_status s = pg::check_marginals(st ? st->last_n : -1, st && st->last_numeric, st ? st->plan.pcg_cap : 0, st ? st->cus : 0, n_nodes, n_query, query,
                                                 cov, n_rows, rows, blocks, opts ? opts->max_workgroups : 0, &G, &h->err))
    return s;
  HIPCHK(h, hipSetDevice(h->device));
  const int n = st->last_n, m = st->last_m;
  const size_t Q = (size_t)n_query, R = (size_t)n_rows;
  const size_t stride = (size_t)pg::kMargNodeDoubles * (size_t)n + (size_t)pg::kMargEdgeDoubles * (size_t)m;
  const size_t need_ws = stride * (size_t)G, need_out = 36 * Q * (1 + R), need_int = Q + R + pg::kMargInts * Q;
  auto grow = [&](auto** p, size_t* cap, size_t count) -> smhip_status {
    if (count <= *cap) return SMHIP_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    void* v = nullptr;
    HIPCHK(h, hipMalloc(&v, count * sizeof(**p)));
    *p = reinterpret_cast<std::remove_reference_t<decltype(*p)>>(v);
    *cap = count;
    return SMHIP_OK;
  };
  if (const smhip_status s = grow(&st->marg_ws, &st->marg_ws_cap, need_ws)) return s;
  if (const smhip_status s = grow(&st->marg_out, &st->marg_out_cap, need_out)) return s;
  if (const smhip_status s = grow(&st->marg_int, &st->marg_int_cap, need_int)) return s;
  hipStream_t s = h->stream;
  pg::Dev d = st->dev;
  d.n = n; d.m = m; d.max_it = 0; d.pcg_cap = st->plan.pcg_cap; d.probe = 3;
  if (!st->last_huber) d.huber = nullptr;
  if (!st->last_info) { d.info_index = nullptr; d.sqrt_info = nullptr; }
  int32_t* d_query = st->marg_int;
  int32_t* d_rows = d_query + Q;
  int32_t* d_info = d_rows + R;
  double* d_cov = st->marg_out;
  double* d_blocks = R ? d_cov + 36 * Q : nullptr;
  HIPCHK(h, hipMemcpyAsync(d_query, query, sizeof(int32_t) * Q, hipMemcpyHostToDevice, s));
  if (R) HIPCHK(h, hipMemcpyAsync(d_rows, rows, sizeof(int32_t) * R, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(pose_graph_solve, dim3(1), dim3(kPgThreads), 0, s, d);
  HIPCHK(h, hipGetLastError());
  int32_t numeric = 0;
  HIPCHK(h, hipMemcpyAsync(&numeric, d.out_i + pg::kOutStop, sizeof(numeric), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  if (numeric == SMHIP_POSE_GRAPH_STOP_NUMERIC) {
    h->err = "pose graph marginals: a pivot of the preconditioner's factorisation at the final poses was not positive; nothing is written";
    return SMHIP_ERR_NO_MATCH;
  }
  hipLaunchKernelGGL(pose_graph_marginals, dim3((unsigned)G), dim3(kPgThreads), 0, s, d, n_query, d_query, n_rows, d_rows, st->marg_ws, stride, d_cov, d_blocks, d_info);
  HIPCHK(h, hipGetLastError());
  st->marg_host_d.resize(need_out);
  st->marg_host_i.resize(pg::kMargInts * Q);
  HIPCHK(h, hipMemcpyAsync(st->marg_host_d.data(), d_cov, sizeof(double) * need_out, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(st->marg_host_i.data(), d_info, sizeof(int32_t) * pg::kMargInts * Q, hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  long long total = 0;
  int longest = 0, capped = 0;
  for (size_t q = 0; q < Q; ++q) {
    const int32_t* i = st->marg_host_i.data() + pg::kMargInts * q;
    total += i[pg::kMargPcg];
    longest = i[pg::kMargPcgMax] > longest ? i[pg::kMargPcgMax] : longest;
    capped |= i[pg::kMargCapped];
  }
  if (stats) { stats->workgroups = G; stats->pcg_iterations = total > INT32_MAX ? INT32_MAX : (int32_t)total; stats->pcg_max_iterations = longest; stats->pcg_cap = st->plan.pcg_cap; }
  if (capped) {
    h->err = "pose graph marginals: a column's solve ended without meeting the tolerance (the cap is " + std::to_string(st->plan.pcg_cap) + " iterations); nothing is written";
    return SMHIP_ERR_NO_MATCH;
  }
  std::memcpy(cov, st->marg_host_d.data(), sizeof(double) * 36 * Q);
  if (R) std::memcpy(blocks, st->marg_host_d.data() + 36 * Q, sizeof(double) * 36 * Q * R);
  return SMHIP_OK;
}

}  // extern "C"
