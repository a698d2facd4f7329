// ndt_ctl_math.h -- the serial end of registrators::Ndt: the 6x6 Newton solve, computeStepLengthMT's helpers and the state
// machine that asks for one computeDerivatives evaluation at a time (pclomp/ndt_omp_impl.hpp:81-171, 633-916).
//
// It stands in a header so that two compilers read the same text: hipcc for ndt_ctl_step (ndt_kernels.hip) and
// g++ -D__HIP_PLATFORM_AMD__ for tests/cpp/test_ndt_ctl.cc, which drives the machine on the host against scripted objectives and
// the solve against a multi-precision pseudo-inverse, without a device.  No HIP runtime call: plain structs and doubles.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace smhip {

struct NdtPose {           // per derivative evaluation
  float T[12];             // final_transformation_ rows 0..2 (float 4x4)
  float j_ang[8][3];       // computeAngleDerivatives (float rows)
  float h_ang[15][3];
  float d1, d2;            // gauss_d1_, gauss_d2_ (d1 kept in double on the host too, see use)
  double d1d, d2d;
  double j_angd[8][3];     // the same rows in double (stock PCL path)
  double h_angd[15][3];
  float res2;              // resolution^2 for the centroid radius test
  int32_t compute_hessian;
};

// ------------------------------------------------------------------------------------------
// The Newton / More-Thuente driver on the device
// ------------------------------------------------------------------------------------------
// computeTransformation (ndt_omp_impl.hpp:81-171) and computeStepLengthMT (:757-916) are sequential 6-vector code around
// computeDerivatives calls.  Each Align is a state machine (NdtCtl) that asks for one evaluation at a time: INIT (:119) -> per
// Newton iteration TRIAL (:809-813) -> MT (the line-search loop's evaluations, :870-878) -> HESS (:912-913, only after a line
// search that looped) -> next iteration.  One round = ndt_derivatives_ctl (every running job's evaluation, grid.y = job) +
// ndt_ctl_step (a workgroup per job: fold of the job's rows in a fixed order, the 6x6 solve, the line-search decision, the next
// pose with its angular derivative tables).  The host only enqueues rounds; it never sees a score or a gradient.
//
// Provenance note: update_interval_mt / trial_value_mt / the ndt_ctl_* transitions follow pclomp/ndt_omp_impl.hpp:633-916 branch
// for branch (same variable roles: a_l, f_l, g_l, a_u, phi_0, d_psi_t, open_interval ...), including the reference's quirk that
// `interval_converged` is computed from the UN-updated interval: the iteration and derivative-call counts the parity tests
// assert depend on that control flow.  Nothing in it is data-parallel; everything it drives is this repository's own code.
struct NdtCtlOpts {
  double step_size, trans_eps;       // computeStepLengthMT's step_max; transformation_epsilon_
  double d1, d2;                     // gauss_d1_, gauss_d2_ (:86-93)
  float res2;                        // resolution^2
  int32_t max_iterations;
  int32_t double_math;               // stock pcl::NormalDistributionsTransform arithmetic (NdtWithGicp): fill the double tables
  int32_t pad_;
};

enum NdtPhase : int32_t { kNdtInit = 0, kNdtTrial = 1, kNdtMt = 2, kNdtHess = 3, kNdtDone = 4, kNdtEvalOnly = 5 };

struct NdtCtl {
  int32_t phase, slot, it, deriv_calls;
  int32_t interval_converged, open_interval, step_iterations, done_round;
  double p[6], x_t[6], dir[6], eval_p[6];
  double sc, g[6], H[36], last_pairs;
  // computeStepLengthMT's locals
  double phi_0, d_phi_0, a_t, a_l, a_u, f_l, g_l, f_u, g_u, phi_t, d_phi_t, psi_t, d_psi_t, step_max, step_min;
  float Tf[16];                      // the pose matrix of the last evaluation asked for = final_transformation_ at the end
  NdtPose pose;                      // the evaluation wanted next
};

struct NdtResult {                   // written to page-locked host memory by the step that ends a job
  float Tf[16];
  double sc, last_pairs;
  int32_t it, deriv_calls, done_round, pad_;
};

constexpr double kMtMu = 1.e-4, kMtNu = 0.9;

__host__ __device__ inline double psi_mt(double a, double f_a, double f_0, double g_0, double mu) { return f_a - f_0 - mu * g_0 * a; }     // ndt_omp.h auxilaryFunction_PsiMT
__host__ __device__ inline double dpsi_mt(double g_a, double g_0, double mu) { return g_a - mu * g_0; }

__host__ __device__ inline bool update_interval_mt(double& a_l, double& f_l, double& g_l, double& a_u, double& f_u, double& g_u, double a_t, double f_t, double g_t) {   // :633-670
  if (f_t > f_l) { a_u = a_t; f_u = f_t; g_u = g_t; return false; }
  else if (g_t * (a_l - a_t) > 0) { a_l = a_t; f_l = f_t; g_l = g_t; return false; }
  else if (g_t * (a_l - a_t) < 0) { a_u = a_l; f_u = f_l; g_u = g_l; a_l = a_t; f_l = f_t; g_l = g_t; return false; }
  return true;
}

__host__ __device__ inline double trial_value_mt(double a_l, double f_l, double g_l, double a_u, double f_u, double g_u, double a_t, double f_t, double g_t) {   // :674-753
  if (f_t > f_l) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t));
    return fabs(a_c - a_l) < fabs(a_q - a_l) ? a_c : 0.5 * (a_q + a_c);
  } else if (g_t * g_l < 0) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    return fabs(a_c - a_t) >= fabs(a_s - a_t) ? a_c : a_s;
  } else if (fabs(g_t) <= fabs(g_l)) {
    const double z = 3 * (f_t - f_l) / (a_t - a_l) - g_t - g_l;
    const double w = sqrt(z * z - g_t * g_l);
    const double a_c = a_l + (a_t - a_l) * (w - g_l - z) / (g_t - g_l + 2 * w);
    const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
    const double nxt = fabs(a_c - a_t) < fabs(a_s - a_t) ? a_c : a_s;
    return a_t > a_l ? fmin(a_t + 0.66 * (a_u - a_t), nxt) : fmax(a_t + 0.66 * (a_u - a_t), nxt);
  }
  const double z = 3 * (f_t - f_u) / (a_t - a_u) - g_t - g_u;
  const double w = sqrt(z * z - g_t * g_u);
  return a_u + (a_t - a_u) * (w - g_u - z) / (g_t - g_u + 2 * w);
}

// Eigen::JacobiSVD<Matrix6d>(H, FullU | FullV).solve(b) (:127-129) = the pseudo-inverse applied to b.  For a matrix of full
// numerical rank that is H^-1 b, formed here by Gaussian elimination with partial pivoting (a few hundred dependent
// instructions on one lane; a Jacobi SVD is several thousand, on the critical path of every round).  The fast path is taken only
// where it provably is the pseudo-inverse: where an upper bound on cond_inf(H), read off the factors, is below 1e10 (see
// ndt_solve6).  Everywhere else the one-sided Jacobi SVD below decides which directions count, with JacobiSVD's threshold.
__host__ __device__ inline __noinline__ void svd_solve6(const double* H /*row-major*/, const double* b, double* x) {
  double A[36], V[36];
  for (int i = 0; i < 36; ++i) { A[i] = H[i]; V[i] = (i % 7 == 0) ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 6; ++p)
      for (int q = p + 1; q < 6; ++q) {
        double app = 0, aqq = 0, apq = 0;
        for (int k = 0; k < 6; ++k) { app += A[6 * k + p] * A[6 * k + p]; aqq += A[6 * k + q] * A[6 * k + q]; apq += A[6 * k + p] * A[6 * k + q]; }
        if (fabs(apq) <= 1e-300 || fabs(apq) <= 1e-16 * sqrt(app * aqq)) continue;
        rotated = true;
        const double zeta = (aqq - app) / (2.0 * apq);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int k = 0; k < 6; ++k) {
          const double ap = A[6 * k + p], aq = A[6 * k + q];
          A[6 * k + p] = c * ap - s * aq; A[6 * k + q] = s * ap + c * aq;
          const double vp = V[6 * k + p], vq = V[6 * k + q];
          V[6 * k + p] = c * vp - s * vq; V[6 * k + q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  double sig[6], smax = 0;
  for (int j = 0; j < 6; ++j) { double s = 0; for (int k = 0; k < 6; ++k) s += A[6 * k + j] * A[6 * k + j]; sig[j] = sqrt(s); smax = fmax(smax, sig[j]); }
  const double thr = 2.220446049250313e-16 * 6 * smax;
  for (int i = 0; i < 6; ++i) x[i] = 0;
  for (int j = 0; j < 6; ++j) {
    if (!(sig[j] > thr)) continue;
    double ub = 0;                                   // u_j . b with u_j = A[:, j] / sig_j
    for (int k = 0; k < 6; ++k) ub += A[6 * k + j] * b[k];
    ub /= sig[j] * sig[j];
    for (int i = 0; i < 6; ++i) x[i] += V[6 * i + j] * ub;
  }
}

__host__ __device__ inline void ndt_solve6(const double* H /*row-major*/, const double* b, double* x) {
  double A[6][7];
  double hmax = 0;                                     // |H|_inf, the largest row sum
  for (int i = 0; i < 6; ++i) {
    double row = 0;
    for (int j = 0; j < 6; ++j) { A[i][j] = H[6 * i + j]; row += fabs(A[i][j]); }
    A[i][6] = b[i];
    hmax = row > hmax ? row : hmax;
  }
  double rinv[6];                                      // 1 / |pivot|
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    double best = fabs(A[c][c]);
#pragma unroll
    for (int r = c + 1; r < 6; ++r) { const double v = fabs(A[r][c]); if (v > best) { best = v; piv = r; } }
    if (!(best > 0) || !(best < 1.7976931348623157e308)) { ok = false; break; }
#pragma unroll
    for (int r = c + 1; r < 6; ++r)
      if (r == piv) {
#pragma unroll
        for (int j = 0; j < 7; ++j) { const double t = A[c][j]; A[c][j] = A[r][j]; A[r][j] = t; }
      }
    const double ip = 1.0 / A[c][c];
    rinv[c] = fabs(ip);
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double f = A[r][c] * ip;
#pragma unroll
      for (int j = c + 1; j < 7; ++j) A[r][j] -= f * A[c][j];
    }
  }
  // Conditioning, not pivot ratio, decides: the pivots of a matrix with a singular value below JacobiSVD's threshold can all stay
  // within ten decades (two pivots of 1e-8 hide one singular value of 1e-17).  P H = L U with |l_ij| <= 1, so |L^-1|_inf <= 2^5;
  // |U^-1|_inf <= max z, z solving the comparison system |u_rr| z_r = 1 + sum_{j > r} |u_rj| z_j.  Below 1e10 the smallest
  // singular value is at least sigma_max / 6e10: far above 6 eps sigma_max, the elimination's answer IS the pseudo-inverse's.
  // (A NaN in H never gets here: it has reached a pivot, and `ok` is false.)
  double cond = 0;
  if (ok) {
    double z[6], zmax = 0;
#pragma unroll
    for (int r = 5; r >= 0; --r) {
      double sacc = 1.0;
#pragma unroll
      for (int j = r + 1; j < 6; ++j) sacc += fabs(A[r][j]) * z[j];
      z[r] = sacc * rinv[r];
      zmax = z[r] > zmax ? z[r] : zmax;
    }
    cond = hmax * 32.0 * zmax;
  }
  if (!ok || !(cond < 1e10)) { svd_solve6(H, b, x); return; }
#pragma unroll
  for (int r = 5; r >= 0; --r) {
    double sacc = A[r][6];
#pragma unroll
    for (int j = r + 1; j < 6; ++j) sacc -= A[r][j] * x[j];
    x[r] = sacc / A[r][r];
  }
}

// ---- the transitions (one lane).  They end by asking for an evaluation at j.eval_p (phase kNdtTrial / kNdtMt: a new pose matrix
// is due; kNdtHess: the same pose once more, Hessian only) or with kNdtDone.
__host__ __device__ inline void ndt_ctl_request(NdtCtl& j, const double* x, bool hess, int32_t ph) {
  for (int i = 0; i < 6; ++i) j.eval_p[i] = x[i];
  j.pose.compute_hessian = hess ? 1 : 0;
  j.phase = ph;
}

__host__ __device__ inline __noinline__ void ndt_ctl_newton(NdtCtl& j, const NdtCtlOpts& o);

__host__ __device__ inline void ndt_ctl_finish_iteration(NdtCtl& j, const NdtCtlOpts& o) {
  const double dp_norm = j.a_t;                                                    // :142
  for (int i = 0; i < 6; ++i) j.p[i] += j.dir[i] * dp_norm;                        // :143, :152
  const bool converged = j.it > o.max_iterations || (j.it && fabs(dp_norm) < o.trans_eps);   // :158-162
  j.it++;                                                                          // :164
  if (converged) { j.phase = kNdtDone; return; }
  ndt_ctl_newton(j, o);
}

// the line-search loop's head (:867): another trial value, the closing Hessian, or the end of the iteration
__host__ __device__ inline void ndt_ctl_mt_continue(NdtCtl& j, const NdtCtlOpts& o) {
  if (!j.interval_converged && j.step_iterations < 10 && !(j.psi_t <= 0 && j.d_phi_t <= -kMtNu * j.d_phi_0)) {
    j.a_t = j.open_interval ? trial_value_mt(j.a_l, j.f_l, j.g_l, j.a_u, j.f_u, j.g_u, j.a_t, j.psi_t, j.d_psi_t)
                            : trial_value_mt(j.a_l, j.f_l, j.g_l, j.a_u, j.f_u, j.g_u, j.a_t, j.phi_t, j.d_phi_t);
    j.a_t = fmax(fmin(j.a_t, j.step_max), j.step_min);
    for (int i = 0; i < 6; ++i) j.x_t[i] = j.p[i] + j.dir[i] * j.a_t;
    ndt_ctl_request(j, j.x_t, false, kNdtMt);
    return;
  }
  if (j.step_iterations) { ndt_ctl_request(j, j.x_t, true, kNdtHess); return; }       // :912-913
  ndt_ctl_finish_iteration(j, o);
}

// one Newton iteration up to its first evaluation (:121-141, :757-813)
__host__ __device__ inline __noinline__ void ndt_ctl_newton(NdtCtl& j, const NdtCtlOpts& o) {
  for (;;) {
    double mg[6], dp[6];
    for (int i = 0; i < 6; ++i) mg[i] = -j.g[i];
    ndt_solve6(j.H, mg, dp);                                                           // :127-129
    double dp_norm = 0;
    for (int i = 0; i < 6; ++i) dp_norm += dp[i] * dp[i];
    dp_norm = sqrt(dp_norm);
    if (dp_norm == 0 || dp_norm != dp_norm) { j.phase = kNdtDone; return; }        // :134-139
    for (int i = 0; i < 6; ++i) j.dir[i] = dp[i] / dp_norm;                        // :141
    // ---- computeStepLengthMT(p, dir, dp_norm, step_size, trans_eps / 2, ...) :757-916
    const double step_init = dp_norm;
    j.step_max = o.step_size; j.step_min = o.trans_eps / 2;
    j.phi_0 = -j.sc;
    j.d_phi_0 = 0;
    for (int i = 0; i < 6; ++i) j.d_phi_0 -= j.g[i] * j.dir[i];
    j.a_t = 0;
    bool skip = false;
    if (j.d_phi_0 >= 0) {
      if (j.d_phi_0 == 0) skip = true;
      else { j.d_phi_0 *= -1; for (int i = 0; i < 6; ++i) j.dir[i] = -j.dir[i]; }
    }
    if (!skip) {
      j.a_l = 0; j.a_u = 0;
      j.f_l = psi_mt(j.a_l, j.phi_0, j.phi_0, j.d_phi_0, kMtMu); j.g_l = dpsi_mt(j.d_phi_0, j.d_phi_0, kMtMu);
      j.f_u = j.f_l; j.g_u = j.g_l;
      j.interval_converged = (j.step_max - j.step_min) > 0 ? 1 : 0;                // :795 (sic: the loop never runs with the wrapper's settings)
      j.open_interval = 1;
      j.step_iterations = 0;
      j.a_t = fmax(fmin(step_init, j.step_max), j.step_min);
      for (int i = 0; i < 6; ++i) j.x_t[i] = j.p[i] + j.dir[i] * j.a_t;
      ndt_ctl_request(j, j.x_t, true, kNdtTrial);                                  // :803-813
      return;
    }
    // d_phi_0 == 0: no step; the iteration ends where it began
    const bool converged = j.it > o.max_iterations || (j.it && fabs(j.a_t) < o.trans_eps);
    j.it++;
    if (converged) { j.phase = kNdtDone; return; }
  }
}

// the evaluation the job asked for has come back: out = score, gradient, hessian (36), pair count
__host__ __device__ inline void ndt_ctl_result(NdtCtl& j, const double* out, const NdtCtlOpts& o) {
  j.deriv_calls++;
  j.last_pairs = out[43];
  switch (j.phase) {
    case kNdtInit:
      j.sc = out[0];
      for (int i = 0; i < 6; ++i) j.g[i] = out[1 + i];
      for (int i = 0; i < 36; ++i) j.H[i] = out[7 + i];
      ndt_ctl_newton(j, o);
      break;
    case kNdtTrial:
      j.sc = out[0];
      for (int i = 0; i < 6; ++i) j.g[i] = out[1 + i];
      for (int i = 0; i < 36; ++i) j.H[i] = out[7 + i];
      j.phi_t = -j.sc; j.d_phi_t = 0;
      for (int i = 0; i < 6; ++i) j.d_phi_t -= j.g[i] * j.dir[i];
      j.psi_t = psi_mt(j.a_t, j.phi_t, j.phi_0, j.d_phi_0, kMtMu); j.d_psi_t = dpsi_mt(j.d_phi_t, j.d_phi_0, kMtMu);
      ndt_ctl_mt_continue(j, o);
      break;
    case kNdtMt:
      j.sc = out[0];
      for (int i = 0; i < 6; ++i) j.g[i] = out[1 + i];                             // (no Hessian in the loop, :872)
      j.phi_t = -j.sc; j.d_phi_t = 0;
      for (int i = 0; i < 6; ++i) j.d_phi_t -= j.g[i] * j.dir[i];
      j.psi_t = psi_mt(j.a_t, j.phi_t, j.phi_0, j.d_phi_0, kMtMu); j.d_psi_t = dpsi_mt(j.d_phi_t, j.d_phi_0, kMtMu);
      if (j.open_interval && (j.psi_t <= 0 && j.d_psi_t >= 0)) {
        j.open_interval = 0;
        j.f_l = j.f_l + j.phi_0 - kMtMu * j.d_phi_0 * j.a_l; j.g_l = j.g_l + kMtMu * j.d_phi_0;
        j.f_u = j.f_u + j.phi_0 - kMtMu * j.d_phi_0 * j.a_u; j.g_u = j.g_u + kMtMu * j.d_phi_0;
      }
      j.interval_converged = (j.open_interval ? update_interval_mt(j.a_l, j.f_l, j.g_l, j.a_u, j.f_u, j.g_u, j.a_t, j.psi_t, j.d_psi_t)
                                              : update_interval_mt(j.a_l, j.f_l, j.g_l, j.a_u, j.f_u, j.g_u, j.a_t, j.phi_t, j.d_phi_t)) ? 1 : 0;
      j.step_iterations++;
      ndt_ctl_mt_continue(j, o);
      break;
    case kNdtHess:
      for (int i = 0; i < 36; ++i) j.H[i] = out[7 + i];                            // the Hessian alone: score and gradient stay the loop's last
      ndt_ctl_finish_iteration(j, o);
      break;
    default:
      break;
  }
}

}  // namespace smhip
