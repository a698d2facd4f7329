// smhip/edge_information.h -- from the information of an alignment (smhip_icp_information, include/smhip.h) to the square-root
// information of a pose-graph edge.  Header-only, host-only: touches no device and needs nothing but the C++ library and the matcher
// layer's AlignInformation (smhip/align_information.h: the C ABI's struct as a value).
//
// The reference weighs every scan-match edge with the same constants, 0.1 rad and 0.15 m on every axis (isam_optimizer.cc:80-83:
// FrameMatchSigmas / LoopClosureSigmas below), whether the two clouds were a city block or a corridor with nothing along the
// direction of travel.  The matcher's point-to-plane normal matrix H = sum J J^T knows the difference: it is rank-deficient exactly
// where the geometry does not constrain the pose.  MakeEdgeInformation combines the two as covariances ADDING: the fixed sigmas stay
// a floor on the uncertainty and the geometry can only add to it.
//
//   sigma2     = max(sum_r2 / (kept - 6), min_residual_sigma^2)           (kept <= 6: every direction counts as unobserved)
//   Lambda_icp = information_scale * H / sigma2                            the Gauss-Newton information of the alignment
//   W          = diag(1 / floor),  Hw = W^-1 Lambda_icp W^-1               dimensionless: the alignment's information in units of the floor's
//   Hw         = Q diag(h) Q^T                                             cyclic Jacobi in f64, eigenvalues ascending
//   g_k        = max(h_k / (1 + h_k), 1 / max_inflation^2)
//   L          = diag(sqrt(g)) Q^T W,   the edge's information = L^T L = W Q diag(g) Q^T W
//
// (Sigma_floor + Sigma_icp)^-1 = W Q diag(h / (1 + h)) Q^T W: a direction the clouds pin down (h >> 1) gets the reference's sigma
// back to within 1/h; one they do not see is inflated up to max_inflation times the fixed sigma and never beyond, so L^T L stays
// positive definite.  The tangent convention is the pose graph's BETWEEN residual (smhip.h, "Pose graph": rotation first).
//
// The defaults are OPTIONS, not measurements.  0.02 m is the range noise of the sensor class the synthetic generator models;
// information_scale = 1 takes the Gauss-Newton covariance at face value, which is known to be optimistic for correlated points --
// the scale is the knob, and `strength` (h) is reported so that a user can set it.  Nobody has measured which scale serves a real
// drive best.
#ifndef SMHIP_EDGE_INFORMATION_H_
#define SMHIP_EDGE_INFORMATION_H_

#include <array>
#include <cmath>
#include <cstdint>

#include "align_information.h"

namespace smhip {
namespace back_end {

using Sigmas = std::array<double, 6>;                                      // rotation first, as gtsam::Pose3
inline Sigmas FrameMatchSigmas() { return {0.1, 0.1, 0.1, 0.15, 0.15, 0.15}; }    // frame_match_noise_model_, isam_optimizer.cc:80-81
inline Sigmas LoopClosureSigmas() { return {0.1, 0.1, 0.1, 0.15, 0.15, 0.15}; }   // loop_closure_noise_model_, :82-83

// the matcher layer's value (smhip/align_information.h), under this layer's name too
using registrator::AlignInformation;
using registrator::FromAbi;

struct EdgeInformationOptions {
  Sigmas floor = FrameMatchSigmas();     // the uncertainty no geometry can go below
  double min_residual_sigma = 0.02;      // metres: the sensor's range noise (an option, not a measurement)
  double information_scale = 1.0;        // 1 = the Gauss-Newton covariance at face value (optimistic for correlated points)
  double max_inflation = 100.0;          // an unobserved direction's sigma is at most this many times the floor's
};

struct EdgeInformation {
  std::array<double, 36> sqrt_information{};   // row-major L; the edge's information is L^T L
  std::array<double, 6> strength{};            // h, ascending
  std::array<double, 6> weakest{};             // the tangent direction of the smallest h: its eigenvector q mapped back through W (the x with
                                               // W x = q), unit length, its largest component positive
  double residual_sigma = 0.0;
  int kept = 0;
};

// Eigen-decomposition of the symmetric 6x6 A (row-major; its upper triangle is read): A = Q diag(w) Q^T, w ascending, column k of
// Q (Q[6 * r + k]) the eigenvector of w[k].  Cyclic Jacobi in f64: sweeps over (p, q), p < q, row by row, each rotation annihilating
// A_pq, until a sweep finds nothing above 1e-300 + 2^-104 of the diagonal's scale or 64 sweeps are done; then a stable selection
// sort.  No data-dependent order anywhere: two calls give the same bits.
inline void JacobiEigen6(const std::array<double, 36>& A_in, std::array<double, 6>* w, std::array<double, 36>* Q) {
  double A[6][6], V[6][6];
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) { A[r][c] = r <= c ? A_in[6 * r + c] : A_in[6 * c + r]; V[r][c] = r == c ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int p = 0; p < 6; ++p) {
      diag += A[p][p] * A[p][p];
      for (int q = p + 1; q < 6; ++q) off += A[p][q] * A[p][q];
    }
    if (!(off > 1.0e-300 + 2.4e-63 * diag)) break;          // off-diagonal norm below 2^-104 of the diagonal's, squared
    for (int p = 0; p < 6; ++p)
      for (int q = p + 1; q < 6; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 6; ++k) {                         // A <- A G
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 6; ++k) {                         // A <- G^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        A[p][q] = 0.0; A[q][p] = 0.0;
        for (int k = 0; k < 6; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int order[6] = {0, 1, 2, 3, 4, 5};
  for (int a = 0; a < 6; ++a) {
    int best = a;
    for (int b = a + 1; b < 6; ++b) if (A[order[b]][order[b]] < A[order[best]][order[best]]) best = b;
    const int o = order[best];
    for (int b = best; b > a; --b) order[b] = order[b - 1];   // stable: equal eigenvalues keep their index order
    order[a] = o;
  }
  for (int k = 0; k < 6; ++k) {
    (*w)[k] = A[order[k]][order[k]];
    for (int r = 0; r < 6; ++r) (*Q)[6 * r + k] = V[r][order[k]];
  }
}

inline EdgeInformation MakeEdgeInformation(const AlignInformation& info, const EdgeInformationOptions& options = EdgeInformationOptions()) {
  EdgeInformation out;
  out.kept = info.kept;
  const bool observed = info.kept > 6;
  const double floor2 = options.min_residual_sigma * options.min_residual_sigma;
  double sigma2 = floor2;
  if (observed) sigma2 = std::fmax(info.sum_r2 / static_cast<double>(info.kept - 6), floor2);
  out.residual_sigma = std::sqrt(sigma2);
  std::array<double, 36> Hw{};
  bool finite = observed && sigma2 > 0.0 && std::isfinite(sigma2);
  if (finite)
    for (int r = 0; r < 6; ++r)
      for (int c = r; c < 6; ++c) {
        const double v = options.information_scale * 0.5 * (info.H[6 * r + c] + info.H[6 * c + r]) / sigma2 * options.floor[r] * options.floor[c];
        finite = finite && std::isfinite(v);
        Hw[6 * r + c] = v; Hw[6 * c + r] = v;
      }
  if (!finite) Hw.fill(0.0);                                  // nothing observed: the floor inflated in every direction
  std::array<double, 6> h;
  std::array<double, 36> Q;
  JacobiEigen6(Hw, &h, &Q);
  const double g_min = 1.0 / (options.max_inflation * options.max_inflation);
  for (int k = 0; k < 6; ++k) {
    const double hk = std::fmax(h[k], 0.0);                   // (a semi-definite matrix's zero eigenvalues may come out as -1e-17)
    out.strength[k] = hk;
    const double g = std::sqrt(std::fmax(hk / (1.0 + hk), g_min));
    for (int c = 0; c < 6; ++c) out.sqrt_information[6 * k + c] = g * Q[6 * c + k] / options.floor[c];
  }
  double norm2 = 0.0;
  int big = 0;
  for (int c = 0; c < 6; ++c) {
    out.weakest[c] = Q[6 * c + 0] * options.floor[c];       // x with W x = q_0: x^T Lambda_icp x / x^T W^2 x = h_0
    norm2 += out.weakest[c] * out.weakest[c];
  }
  for (int c = 1; c < 6; ++c) if (std::fabs(out.weakest[c]) > std::fabs(out.weakest[big])) big = c;
  const double scale = (out.weakest[big] < 0.0 ? -1.0 : 1.0) / std::sqrt(norm2);
  for (int c = 0; c < 6; ++c) out.weakest[c] *= scale;
  return out;
}

}  // namespace back_end
}  // namespace smhip

#endif  // SMHIP_EDGE_INFORMATION_H_
