// pose_graph_kernel.h -- the pose-graph optimiser's whole loop ("Pose graph"; tests/pose_graph_ref.py), written
// once against a small execution context: Ctx gives the thread's index, the number of threads, a barrier and two reductions.
// smhip_pose_graph.hip instantiates it with one workgroup of 1024 threads inside ONE kernel; HostCtx below is one thread with
// empty barriers, which runs the same code on a CPU (tests/cpp/test_pose_graph.cc, and a debugger when a result is in doubt).
//
// Every phase is "items dealt to the threads by a stride, then a barrier"; all state is in global memory (L2-resident at these
// sizes).  Scalars that steer the loop (costs, dot products, the largest step component) come out of the reductions with the same
// bits in every thread, so all threads take the same branches and meet at the same barriers.  Every loop has a bound from the
// sizes or the options; nothing waits on memory.
//
// Poses and measurements are 12 doubles here: the rotation row-major, then the translation.  A factor is a BETWEEN, a PRIOR, a
// POINT (include/smhip.h, "Factor kinds"; tests/pose_graph_gps_ref.py) or a HANDEYE ("Odometry calibration factor";
// tests/pose_graph_calib_ref.py); whatever its kind it has an index pair, 12 doubles of
// data, 6 inverse sigmas and 6 rows of whitened A, B and residual, so only edge_cost and linearize_edge look at the kind.
// A BETWEEN may carry a full 6x6 square-root information L in place of its six inverse sigmas (Dev::info_index, Dev::sqrt_info).
// Any factor may carry a Huber threshold (include/smhip.h, "Robust factors"; tests/pose_graph_robust_ref.py): the same two
// functions turn s_f^2 into the cost term and the rows into the weighted rows, and nothing else of the loop knows.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/smhip.h"

#if defined(__HIPCC__)
#define PG_HD __host__ __device__ inline
#else
#define PG_HD inline
#endif

namespace smhip {
namespace pose_graph {

constexpr double kStepTol = 1.0e-10, kCostTol = 1.0e-12, kCostNoise = 1.0e-11, kPcgTol = 1.0e-8, kMarginalPcgTol = 1.0e-10, kLambdaFirst = 1.0e-4, kLambdaMax = 1.0e8;
enum { kOutInitial = 0, kOutFinal = 1, kOutLambda = 2, kOutDoubles = 3 };
enum { kOutStop = 0, kOutIterations = 1, kOutAccepted = 2, kOutRejected = 3, kOutPcg = 4, kOutPcgMax = 5, kOutInts = 6 };
enum { kMargPcg = 0, kMargPcgMax = 1, kMargCapped = 2, kMargInts = 3 };       // per query: iterations of its six solves, the longest, a column whose solve ended without meeting the stop rule (at the cap or otherwise)
constexpr int kMargNodeDoubles = 7 * 6, kMargEdgeDoubles = 6;                  // a workgroup's slice of the marginals' workspace: x r z p q b g per node, u per edge

struct Dev {
  int n = 0, m = 0;                       // nodes, edges
  int max_it = 0, pcg_cap = 0;
  int pcg_budget = 0;                     // conjugate-gradient iterations of the whole launch (SMHIP_POSE_GRAPH_MAX_PCG_TOTAL)
  int probe = 0;                          // 1: first linearisation, gradient and M^-1 v only (smhip_pose_graph_last)
                                          // 2: the report at the poses in cur, left there by the last loop (smhip_pose_graph_last_robust)
                                          // 3: linearise at cur, assemble and factor at lambda = 0, nothing else: what pose_graph_marginals reads
  // per node
  const double* pose0 = nullptr;          // 12: the poses as given
  double *cur = nullptr, *cand = nullptr; // 12
  double *Hkk = nullptr, *C = nullptr;    // 36: diagonal block of H; block (k, k + 1) of H (chain edges only)
  double *D = nullptr, *U = nullptr, *Dinv = nullptr, *Wm = nullptr, *Wp = nullptr;   // 36: the cyclic reduction's factors
  double *g = nullptr, *x = nullptr, *r = nullptr, *z = nullptr, *p = nullptr, *q = nullptr, *b = nullptr;   // 6
  const int32_t *fixed = nullptr, *csr_off = nullptr, *csr_edge = nullptr;
  // per edge
  const int32_t* ij = nullptr;            // 2
  const int32_t* kind = nullptr;          // SMHIP_POSE_GRAPH_FACTOR_*; nullptr: every factor is a BETWEEN
  const double* Z = nullptr;              // 12: BETWEEN the measurement, PRIOR the pose P, POINT the lever (0..2) and the point (3..5), HANDEYE the odometer's pose
  const double* sinv = nullptr;           // 6: 1 / sigma (POINT reads the first three)
  double *A = nullptr, *B = nullptr;      // 36, row-major, whitened
  double *rw = nullptr, *u = nullptr;     // 6: whitened residual; A p_i + B p_j
  const double* huber = nullptr;          // 1: the Huber threshold k_f, 0 = none; nullptr: no threshold anywhere ("Robust factors")
  double* wgt = nullptr;                  // 1: the weight w_f of the last linearisation (1, or k_f / s_f); nullptr: not kept
  double *rep_s = nullptr, *rep_c = nullptr;   // 1: the report's s_f and cost term (its weight goes to wgt)
  const int32_t* info_index = nullptr;    // 1: >= 0: the BETWEEN factor is whitened by the 6x6 L at sqrt_info + 36 * index in place of its sinv (rw = L e,
  const double* sqrt_info = nullptr;      //    A_w = L A, B_w = L B, s_f^2 = |L e|^2; DESIGN.md section 6, "Edge information"); both nullptr: no factor has one
  // probe
  const double* v = nullptr;
  double* minv = nullptr;
  double* out_d = nullptr;
  int32_t* out_i = nullptr;
};

struct HostCtx {
  int tid() const { return 0; }
  int nthreads() const { return 1; }
  void sync() const {}
  double sum(double v) const { return v; }
  double max(double v) const { return v; }
};

// ---- SO(3) -------------------------------------------------------------------------------------------------------------

PG_HD void exp_so3(const double* w, double* R) {
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(t2);
  double a, b;
  if (th < 1.0e-4) { a = 1.0 - t2 / 6.0; b = 0.5 - t2 / 24.0; }
  else { a = sin(th) / th; b = (1.0 - cos(th)) / t2; }
  // I + a K + b K^2,  K^2 = w w^T - |w|^2 I
  R[0] = 1.0 + b * (w[0] * w[0] - t2); R[1] = -a * w[2] + b * w[0] * w[1];  R[2] = a * w[1] + b * w[0] * w[2];
  R[3] = a * w[2] + b * w[0] * w[1];   R[4] = 1.0 + b * (w[1] * w[1] - t2); R[5] = -a * w[0] + b * w[1] * w[2];
  R[6] = -a * w[1] + b * w[0] * w[2];  R[7] = a * w[0] + b * w[1] * w[2];   R[8] = 1.0 + b * (w[2] * w[2] - t2);
}

// theta = atan2(|w|, c) with w = vee(R - R^T) / 2 = sin(theta) axis and c = (tr R - 1) / 2.  c > -0.5: (theta / sin theta) w, by its
// series below |w| = 1e-4.  Towards pi, where sin(theta) vanishes: the axis from the symmetric part, a a^T = ((R + R^T) / 2 - c I) /
// (1 - c), the column of its largest diagonal entry (the first of equals), signed like w.
PG_HD void log_so3(const double* R, double* phi) {
  const double w[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
  const double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  const double s = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double th = atan2(s, c);
  if (c > -0.5) {
    const double t2 = th * th;
    const double k = s < 1.0e-4 ? 1.0 + t2 / 6.0 + 7.0 * t2 * t2 / 360.0 : th / s;
    phi[0] = k * w[0]; phi[1] = k * w[1]; phi[2] = k * w[2];
    return;
  }
  const double d[3] = {(R[0] - c) / (1.0 - c), (R[4] - c) / (1.0 - c), (R[8] - c) / (1.0 - c)};
  int k = 0;
  if (d[1] > d[k]) k = 1;
  if (d[2] > d[k]) k = 2;
  double a[3];
  const double root = sqrt(d[k]);
  for (int r = 0; r < 3; ++r) a[r] = r == k ? root : 0.5 * (R[3 * r + k] + R[3 * k + r]) / (1.0 - c) / root;
  const double sg = a[0] * w[0] + a[1] * w[1] + a[2] * w[2] < 0.0 ? -th : th;
  phi[0] = sg * a[0]; phi[1] = sg * a[1]; phi[2] = sg * a[2];
}

// I + hat / 2 + c hat^2,  c = (1 - (theta/2) cot(theta/2)) / theta^2: no division by sin(theta), pi is an ordinary point
PG_HD void jr_inv(const double* f, double* J) {
  const double t2 = f[0] * f[0] + f[1] * f[1] + f[2] * f[2], th = sqrt(t2);
  double c;
  if (th < 1.0e-2) c = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0;
  else { const double h = 0.5 * th; c = (1.0 - h * cos(h) / sin(h)) / t2; }
  J[0] = 1.0 + c * (f[0] * f[0] - t2);    J[1] = -0.5 * f[2] + c * f[0] * f[1];  J[2] = 0.5 * f[1] + c * f[0] * f[2];
  J[3] = 0.5 * f[2] + c * f[0] * f[1];    J[4] = 1.0 + c * (f[1] * f[1] - t2);   J[5] = -0.5 * f[0] + c * f[1] * f[2];
  J[6] = -0.5 * f[1] + c * f[0] * f[2];   J[7] = 0.5 * f[0] + c * f[1] * f[2];   J[8] = 1.0 + c * (f[2] * f[2] - t2);
}

// ---- one edge ------------------------------------------------------------------------------------------------------------

// e = [Log(Rz^T Rij); Rz^T (tij - tz)], with Rij = Ri^T Rj, tij = Ri^T (tj - ti) and RE = Rz^T Rij handed back
PG_HD void edge_error(const double* Xi, const double* Xj, const double* Z, double* e, double* Rij, double* tij, double* RE) {
  const double d[3] = {Xj[9] - Xi[9], Xj[10] - Xi[10], Xj[11] - Xi[11]};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) Rij[3 * a + b] = Xi[a] * Xj[b] + Xi[3 + a] * Xj[3 + b] + Xi[6 + a] * Xj[6 + b];
    tij[a] = Xi[a] * d[0] + Xi[3 + a] * d[1] + Xi[6 + a] * d[2];
  }
  const double dz[3] = {tij[0] - Z[9], tij[1] - Z[10], tij[2] - Z[11]};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) RE[3 * a + b] = Z[a] * Rij[b] + Z[3 + a] * Rij[3 + b] + Z[6 + a] * Rij[6 + b];
    e[3 + a] = Z[a] * dz[0] + Z[3 + a] * dz[1] + Z[6 + a] * dz[2];
  }
  log_so3(RE, e);
}

// POINT: r = R_i (R_j l + t_j) + t_i - z, with p = R_j l + t_j handed back
PG_HD void point_error(const double* Xi, const double* Xj, const double* lz, double* r, double* p) {
  for (int a = 0; a < 3; ++a) p[a] = Xj[3 * a] * lz[0] + Xj[3 * a + 1] * lz[1] + Xj[3 * a + 2] * lz[2] + Xj[9 + a];
  for (int a = 0; a < 3; ++a) r[a] = Xi[3 * a] * p[0] + Xi[3 * a + 1] * p[1] + Xi[3 * a + 2] * p[2] + Xi[9 + a] - lz[3 + a];
}

// HANDEYE: h = T^-1 X T and E = Z^-1 h for the frame node's pose X and the calibration node's pose T; e = [Log(R_E); t_E], with
// R_h, t_h and R_E handed back
PG_HD void handeye_error(const double* X, const double* T, const double* Z, double* e, double* Rh, double* th, double* RE) {
  double M[9], u[3];                                                               // R_X R_T;  R_X t_T + t_X - t_T
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) M[3 * a + b] = X[3 * a] * T[b] + X[3 * a + 1] * T[3 + b] + X[3 * a + 2] * T[6 + b];
    u[a] = X[3 * a] * T[9] + X[3 * a + 1] * T[10] + X[3 * a + 2] * T[11] + X[9 + a] - T[9 + a];
  }
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) Rh[3 * a + b] = T[a] * M[b] + T[3 + a] * M[3 + b] + T[6 + a] * M[6 + b];
    th[a] = T[a] * u[0] + T[3 + a] * u[1] + T[6 + a] * u[2];
  }
  const double dz[3] = {th[0] - Z[9], th[1] - Z[10], th[2] - Z[11]};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) RE[3 * a + b] = Z[a] * Rh[b] + Z[3 + a] * Rh[3 + b] + Z[6 + a] * Rh[6 + b];
    e[3 + a] = Z[a] * dz[0] + Z[3 + a] * dz[1] + Z[6 + a] * dz[2];
  }
  log_so3(RE, e);
}

// the factor's 6x6 L (row-major), or nullptr: whitened by its six inverse sigmas
PG_HD const double* edge_sqrt_info(const Dev& d, int e) {
  if (!d.info_index || d.info_index[e] < 0) return nullptr;
  return d.sqrt_info + 36 * (size_t)d.info_index[e];
}

// A PRIOR on node i around P is the BETWEEN from a constant node at P measured as the identity: the same residual, and that
// factor's B is the PRIOR's only Jacobian.
PG_HD double edge_norm2(const Dev& d, const double* X, int e) {
  const int kind = d.kind ? d.kind[e] : SMHIP_POSE_GRAPH_FACTOR_BETWEEN;
  const double* Xi = X + 12 * (size_t)d.ij[2 * e];
  const double* Xj = X + 12 * (size_t)d.ij[2 * e + 1];
  const double* Z = d.Z + 12 * (size_t)e;
  const double* sinv = d.sinv + 6 * (size_t)e;
  double s = 0.0;
  if (kind == SMHIP_POSE_GRAPH_FACTOR_POINT) {
    double r[3], p[3];
    point_error(Xi, Xj, Z, r, p);
    for (int a = 0; a < 3; ++a) { const double w = r[a] * sinv[a]; s += w * w; }
    return s;
  }
  if (kind == SMHIP_POSE_GRAPH_FACTOR_HANDEYE) {
    double err[6], Rh[9], th[3], RE[9];
    handeye_error(Xi, Xj, Z, err, Rh, th, RE);
    for (int a = 0; a < 6; ++a) { const double w = err[a] * sinv[a]; s += w * w; }
    return s;
  }
  const double eye[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
  const bool prior = kind == SMHIP_POSE_GRAPH_FACTOR_PRIOR;
  double err[6], Rij[9], tij[3], RE[9];
  edge_error(prior ? Z : Xi, Xj, prior ? eye : Z, err, Rij, tij, RE);
  if (const double* L = prior ? nullptr : edge_sqrt_info(d, e)) {
    for (int a = 0; a < 6; ++a) {
      double w = 0.0;
      for (int k = 0; k < 6; ++k) w += L[6 * a + k] * err[k];
      s += w * w;
    }
    return s;
  }
  for (int a = 0; a < 6; ++a) { const double w = err[a] * sinv[a]; s += w * w; }
  return s;
}

// s_f^2 -> the factor's cost term: s_f^2 itself within the threshold (or without one), else 2 k_f s_f - k_f^2, twice the Huber loss
PG_HD double huber_term(const Dev& d, int e, double s2) {
  if (d.huber) {
    const double k = d.huber[e];
    if (k > 0.0 && s2 > k * k) return 2.0 * k * sqrt(s2) - k * k;
  }
  return s2;
}
// ... and its weight
PG_HD double huber_weight(const Dev& d, int e, double s2) {
  if (d.huber) {
    const double k = d.huber[e];
    if (k > 0.0 && s2 > k * k) return k / sqrt(s2);
  }
  return 1.0;
}

PG_HD double edge_cost(const Dev& d, const double* X, int e) { return huber_term(d, e, edge_norm2(d, X, e)); }

PG_HD void linearize_edge_plain(const Dev& d, const double* X, int e) {
  const int kind = d.kind ? d.kind[e] : SMHIP_POSE_GRAPH_FACTOR_BETWEEN;
  const double* Xi = X + 12 * (size_t)d.ij[2 * e];
  const double* Xj = X + 12 * (size_t)d.ij[2 * e + 1];
  const double* Z = d.Z + 12 * (size_t)e;
  const double* sinv = d.sinv + 6 * (size_t)e;
  double* A = d.A + 36 * (size_t)e;
  double* B = d.B + 36 * (size_t)e;
  if (kind == SMHIP_POSE_GRAPH_FACTOR_POINT) {
    double r[3], p[3], RR[9];
    point_error(Xi, Xj, Z, r, p);
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) RR[3 * a + b] = Xi[3 * a] * Xj[b] + Xi[3 * a + 1] * Xj[3 + b] + Xi[3 * a + 2] * Xj[6 + b];          // R_i R_j
    const double hp[9] = {0.0, -p[2], p[1], p[2], 0.0, -p[0], -p[1], p[0], 0.0};
    const double hl[9] = {0.0, -Z[2], Z[1], Z[2], 0.0, -Z[0], -Z[1], Z[0], 0.0};
    for (int a = 0; a < 3; ++a) {
      const double w = sinv[a];
      for (int b = 0; b < 3; ++b) {
        A[6 * a + b] = -w * (Xi[3 * a] * hp[b] + Xi[3 * a + 1] * hp[3 + b] + Xi[3 * a + 2] * hp[6 + b]);                            // -R_i hat(p)
        A[6 * a + 3 + b] = w * Xi[3 * a + b];
        B[6 * a + b] = -w * (RR[3 * a] * hl[b] + RR[3 * a + 1] * hl[3 + b] + RR[3 * a + 2] * hl[6 + b]);                            // -R_i R_j hat(l)
        B[6 * a + 3 + b] = w * RR[3 * a + b];
      }
      d.rw[6 * (size_t)e + a] = r[a] * w;
      d.rw[6 * (size_t)e + 3 + a] = 0.0;
    }
    for (int k = 18; k < 36; ++k) { A[k] = 0.0; B[k] = 0.0; }
    return;
  }
  if (kind == SMHIP_POSE_GRAPH_FACTOR_HANDEYE) {
    // A = B_h Ad(T^-1), B = B_h (I - Ad(h^-1)) with B_h = [Jr^-1, 0; 0, R_E], Ad(G) = [R_G, 0; hat(t_G) R_G, R_G], written out block
    // by block and row by row into memory: Ad(T^-1) = [R_T^T, 0; -R_T^T hat(t_T), R_T^T], Ad(h^-1) = [R_h^T, 0; -R_h^T hat(t_h), R_h^T],
    // R_E R_h^T = R_Z^T, and a row p times hat(t) is the cross product p x t.  Both upper right blocks are zero.
    double err[6], Rh[9], th[3], RE[9], J[9];
    handeye_error(Xi, Xj, Z, err, Rh, th, RE);
    jr_inv(err, J);
    const double* tT = Xj + 9;
    for (int a = 0; a < 3; ++a) {
      const double w = sinv[a], v = sinv[3 + a];
      double p[3];                                                                                                       // row a of R_E R_T^T
      for (int b = 0; b < 3; ++b) p[b] = RE[3 * a] * Xj[3 * b] + RE[3 * a + 1] * Xj[3 * b + 1] + RE[3 * a + 2] * Xj[3 * b + 2];
      const double q[3] = {Z[a], Z[3 + a], Z[6 + a]};                                                                    // row a of R_Z^T
      const double pt[3] = {p[1] * tT[2] - p[2] * tT[1], p[2] * tT[0] - p[0] * tT[2], p[0] * tT[1] - p[1] * tT[0]};
      const double qt[3] = {q[1] * th[2] - q[2] * th[1], q[2] * th[0] - q[0] * th[2], q[0] * th[1] - q[1] * th[0]};
      for (int b = 0; b < 3; ++b) {
        A[6 * a + b] = w * (J[3 * a] * Xj[3 * b] + J[3 * a + 1] * Xj[3 * b + 1] + J[3 * a + 2] * Xj[3 * b + 2]);         // Jr^-1 R_T^T
        A[6 * a + 3 + b] = 0.0;
        A[6 * (3 + a) + b] = -v * pt[b];                                                                                 // -R_E R_T^T hat(t_T)
        A[6 * (3 + a) + 3 + b] = v * p[b];
        B[6 * a + b] = w * (J[3 * a + b] - (J[3 * a] * Rh[3 * b] + J[3 * a + 1] * Rh[3 * b + 1] + J[3 * a + 2] * Rh[3 * b + 2]));   // Jr^-1 (I - R_h^T)
        B[6 * a + 3 + b] = 0.0;
        B[6 * (3 + a) + b] = v * qt[b];                                                                                  // R_Z^T hat(t_h)
        B[6 * (3 + a) + 3 + b] = v * (RE[3 * a + b] - q[b]);                                                             // R_E - R_Z^T
      }
    }
    for (int a = 0; a < 6; ++a) d.rw[6 * (size_t)e + a] = err[a] * sinv[a];
    return;
  }
  const double eye[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
  const bool prior = kind == SMHIP_POSE_GRAPH_FACTOR_PRIOR;
  if (prior) { Xi = Z; Z = eye; double* t = A; A = B; B = t; }                  // (the constant twin's Jacobian is dropped below)
  const double* L = prior ? nullptr : edge_sqrt_info(d, e);
  const double ones[6] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
  if (L) sinv = ones;                                                           // the plain rows first (times one: exact), then L times them
  double err[6], Rij[9], tij[3], RE[9], J[9];
  edge_error(Xi, Xj, Z, err, Rij, tij, RE);
  jr_inv(err, J);
  const double hat[9] = {0.0, -tij[2], tij[1], tij[2], 0.0, -tij[0], -tij[1], tij[0], 0.0};
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      const double w = sinv[a], v = sinv[3 + a];
      A[6 * a + b] = -w * (J[3 * a] * Rij[3 * b] + J[3 * a + 1] * Rij[3 * b + 1] + J[3 * a + 2] * Rij[3 * b + 2]);       // -Jr^-1 Rij^T
      A[6 * a + 3 + b] = 0.0;
      A[6 * (3 + a) + b] = v * (Z[a] * hat[b] + Z[3 + a] * hat[3 + b] + Z[6 + a] * hat[6 + b]);                          // Rz^T hat(tij)
      A[6 * (3 + a) + 3 + b] = -v * Z[3 * b + a];                                                                        // -Rz^T
      B[6 * a + b] = w * J[3 * a + b];
      B[6 * a + 3 + b] = 0.0;
      B[6 * (3 + a) + b] = 0.0;
      B[6 * (3 + a) + 3 + b] = v * RE[3 * a + b];                                                                        // Rz^T Rij
    }
  if (prior) for (int k = 0; k < 36; ++k) A[k] = 0.0;
  if (L) {
    double LA[36], LB[36];
    for (int a = 0; a < 6; ++a) {
      double w = 0.0;
      for (int k = 0; k < 6; ++k) w += L[6 * a + k] * err[k];
      d.rw[6 * (size_t)e + a] = w;
      for (int b = 0; b < 6; ++b) {
        double sa = 0.0, sb = 0.0;
        for (int k = 0; k < 6; ++k) { sa += L[6 * a + k] * A[6 * k + b]; sb += L[6 * a + k] * B[6 * k + b]; }
        LA[6 * a + b] = sa; LB[6 * a + b] = sb;
      }
    }
    for (int k = 0; k < 36; ++k) { A[k] = LA[k]; B[k] = LB[k]; }
    return;
  }
  for (int a = 0; a < 6; ++a) d.rw[6 * (size_t)e + a] = err[a] * sinv[a];
}

// The whitened rows exactly as without thresholds, then -- only where w_f < 1 -- times sqrt(w_f): J^T r becomes the gradient of half
// the robust cost and H the sum of w J^T J (GTSAM's Robust::WhitenSystem).  The plain rows are written first and scaled from
// memory, so that their expressions, and with them their bits, stay what they are without a threshold.
PG_HD void linearize_edge(const Dev& d, const double* X, int e) {
  linearize_edge_plain(d, X, e);
  double* rw = d.rw + 6 * (size_t)e;
  double s2 = 0.0;
  for (int a = 0; a < 6; ++a) s2 += rw[a] * rw[a];                              // (rows 3..5 of a POINT are zero)
  const double w = huber_weight(d, e, s2);
  if (d.wgt) d.wgt[e] = w;
  if (!(w < 1.0)) return;
  const double q = sqrt(w);
  double* A = d.A + 36 * (size_t)e;
  double* B = d.B + 36 * (size_t)e;
  for (int k = 0; k < 36; ++k) { A[k] *= q; B[k] *= q; }
  for (int a = 0; a < 6; ++a) rw[a] *= q;
}

// ---- 6x6 blocks -------------------------------------------------------------------------------------------------------------

// X = D^-1 through the Cholesky factor; false (and X = 0) when a pivot is not positive
PG_HD bool inv6(const double* D, double* X) {
  double L[36], Li[36];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = D[6 * i + j];
      for (int k = 0; k < j; ++k) s -= L[6 * i + k] * L[6 * j + k];
      if (i == j) {
        if (!(s > 0.0) || !(s < 1.0e300)) { for (int k = 0; k < 36; ++k) X[k] = 0.0; return false; }
        L[6 * i + i] = sqrt(s);
      } else {
        L[6 * i + j] = s / L[6 * j + j];
      }
    }
  for (int c = 0; c < 6; ++c)
    for (int i = 0; i < 6; ++i) {
      if (i < c) { Li[6 * i + c] = 0.0; continue; }
      if (i == c) { Li[6 * i + c] = 1.0 / L[6 * i + i]; continue; }
      double s = 0.0;
      for (int k = c; k < i; ++k) s += L[6 * i + k] * Li[6 * k + c];
      Li[6 * i + c] = -s / L[6 * i + i];
    }
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) {
      double s = 0.0;
      for (int k = a > b ? a : b; k < 6; ++k) s += Li[6 * k + a] * Li[6 * k + b];
      X[6 * a + b] = s;
    }
  return true;
}

// out (+)= sign * op(P) Q for row-major 6x6 blocks; tp: P transposed
PG_HD void mm6(double* out, const double* P, bool tp, const double* Q, double sign, bool accumulate) {
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) {
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s += (tp ? P[6 * k + a] : P[6 * a + k]) * Q[6 * k + b];
      out[6 * a + b] = (accumulate ? out[6 * a + b] : 0.0) + sign * s;
    }
}
// out = P Q^T
PG_HD void mmt6(double* out, const double* P, const double* Q) {
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) {
      double s = 0.0;
      for (int k = 0; k < 6; ++k) s += P[6 * a + k] * Q[6 * b + k];
      out[6 * a + b] = s;
    }
}
// y (+)= sign * op(P) x
PG_HD void mv6(double* y, const double* P, bool tp, const double* x, double sign, bool accumulate) {
  for (int a = 0; a < 6; ++a) {
    double s = 0.0;
    for (int k = 0; k < 6; ++k) s += (tp ? P[6 * k + a] : P[6 * a + k]) * x[k];
    y[a] = (accumulate ? y[a] : 0.0) + sign * s;
  }
}

// ---- phases ---------------------------------------------------------------------------------------------------------------

template <class Ctx>
PG_HD double total_cost(const Dev& d, Ctx& c, const double* X) {
  double s = 0.0;
  for (int e = c.tid(); e < d.m; e += c.nthreads()) s += edge_cost(d, X, e);
  return c.sum(s);
}

template <class Ctx>
PG_HD void linearize(const Dev& d, Ctx& c, const double* X) {
  for (int e = c.tid(); e < d.m; e += c.nthreads()) linearize_edge(d, X, e);
  c.sync();
}

// One thread per node gathers its edges in index order: Hkk, g and the chain block C = block (k, k + 1) of H.
template <class Ctx>
PG_HD void assemble(const Dev& d, Ctx& c) {
  for (int k = c.tid(); k < d.n; k += c.nthreads()) {
    double* H = d.Hkk + 36 * (size_t)k;
    double* C = d.C + 36 * (size_t)k;
    double* g = d.g + 6 * (size_t)k;
    for (int a = 0; a < 36; ++a) { H[a] = 0.0; C[a] = 0.0; }
    for (int a = 0; a < 6; ++a) g[a] = 0.0;
    if (d.fixed[k]) { for (int a = 0; a < 6; ++a) H[7 * a] = 1.0; continue; }
    const bool chain = k + 1 < d.n && !d.fixed[k + 1];
    for (int at = d.csr_off[k]; at < d.csr_off[k + 1]; ++at) {
      const int e = d.csr_edge[at], i = d.ij[2 * e], j = d.ij[2 * e + 1];
      const double* A = d.A + 36 * (size_t)e;
      const double* B = d.B + 36 * (size_t)e;
      const double* mine = i == k ? A : B;
      mm6(H, mine, true, mine, 1.0, true);
      mv6(g, mine, true, d.rw + 6 * (size_t)e, 1.0, true);
      if (chain && i == k && j == k + 1) mm6(C, A, true, B, 1.0, true);
      if (chain && j == k && i == k + 1) mm6(C, B, true, A, 1.0, true);
    }
  }
  c.sync();
}

// Block cyclic reduction of M(lambda) = blockdiag((1 + lambda) Hkk) + the chain blocks.  Level s = 1, 2, 4, ...: the active nodes
// are the multiples of s and U_j couples j with j + s; the odd multiples are eliminated (their D^-1 and W- = D^-1 U_{i-s}^T,
// W+ = D^-1 U_i stay for the solves), the even ones take the Schur complements and the coupling to j + 2s.  Node 0 is last.
template <class Ctx>
PG_HD bool factor(const Dev& d, Ctx& c, double lambda) {
  double bad = 0.0;
  for (int k = c.tid(); k < d.n; k += c.nthreads()) {
    const double scale = d.fixed[k] ? 1.0 : 1.0 + lambda;
    for (int a = 0; a < 36; ++a) { d.D[36 * (size_t)k + a] = scale * d.Hkk[36 * (size_t)k + a]; d.U[36 * (size_t)k + a] = d.C[36 * (size_t)k + a]; }
  }
  c.sync();
  for (int s = 1; s < d.n; s <<= 1) {
    for (long long i = s + 2LL * s * c.tid(); i < d.n; i += 2LL * s * c.nthreads()) {
      double* Di = d.Dinv + 36 * (size_t)i;
      if (!inv6(d.D + 36 * (size_t)i, Di)) bad = 1.0;
      mmt6(d.Wm + 36 * (size_t)i, Di, d.U + 36 * (size_t)(i - s));
      if (i + s < d.n) mm6(d.Wp + 36 * (size_t)i, Di, false, d.U + 36 * (size_t)i, 1.0, false);
      else for (int a = 0; a < 36; ++a) d.Wp[36 * (size_t)i + a] = 0.0;
    }
    c.sync();
    for (long long j = 2LL * s * c.tid(); j < d.n; j += 2LL * s * c.nthreads()) {
      double* Dj = d.D + 36 * (size_t)j;
      double* Uj = d.U + 36 * (size_t)j;
      double next[36];
      for (int a = 0; a < 36; ++a) next[a] = 0.0;
      if (j + s < d.n) {
        mm6(Dj, Uj, false, d.Wm + 36 * (size_t)(j + s), -1.0, true);
        if (j + 2LL * s < d.n) mm6(next, Uj, false, d.Wp + 36 * (size_t)(j + s), -1.0, false);
      }
      if (j >= s) mm6(Dj, d.U + 36 * (size_t)(j - s), true, d.Wp + 36 * (size_t)(j - s), -1.0, true);
      for (int a = 0; a < 36; ++a) Uj[a] = next[a];
    }
    c.sync();
  }
  if (c.tid() == 0 && !inv6(d.D, d.Dinv)) bad = 1.0;
  return !(c.max(bad) > 0.0);
}

// out = M^-1 in (in and out may be the same array): the forward sweep up the levels, the root, the backward sweep down
template <class Ctx>
PG_HD void apply_minv(const Dev& d, Ctx& c, const double* in, double* out) {
  for (int k = c.tid(); k < d.n; k += c.nthreads())
    for (int a = 0; a < 6; ++a) d.b[6 * (size_t)k + a] = in[6 * (size_t)k + a];
  c.sync();
  int top = 0;
  for (int s = 1; s < d.n; s <<= 1) {
    top = s;
    for (long long j = 2LL * s * c.tid(); j < d.n; j += 2LL * s * c.nthreads()) {
      double* bj = d.b + 6 * (size_t)j;
      if (j + s < d.n) mv6(bj, d.Wm + 36 * (size_t)(j + s), true, d.b + 6 * (size_t)(j + s), -1.0, true);
      if (j >= s) mv6(bj, d.Wp + 36 * (size_t)(j - s), true, d.b + 6 * (size_t)(j - s), -1.0, true);
    }
    c.sync();
  }
  if (c.tid() == 0) mv6(out, d.Dinv, false, d.b, 1.0, false);
  c.sync();
  for (int s = top; s >= 1; s >>= 1) {
    for (long long i = s + 2LL * s * c.tid(); i < d.n; i += 2LL * s * c.nthreads()) {
      double* oi = out + 6 * (size_t)i;
      double t[6];
      mv6(t, d.Dinv + 36 * (size_t)i, false, d.b + 6 * (size_t)i, 1.0, false);
      mv6(t, d.Wm + 36 * (size_t)i, false, out + 6 * (size_t)(i - s), -1.0, true);
      if (i + s < d.n) mv6(t, d.Wp + 36 * (size_t)i, false, out + 6 * (size_t)(i + s), -1.0, true);
      for (int a = 0; a < 6; ++a) oi[a] = t[a];
    }
    c.sync();
  }
}

// q = (H + lambda blockdiag(H)) p, matrix-free: u_e = A p_i + B p_j per edge, then every node gathers in index order
template <class Ctx>
PG_HD void hmul(const Dev& d, Ctx& c, double lambda, const double* p, double* q) {
  for (int e = c.tid(); e < d.m; e += c.nthreads()) {
    double* u = d.u + 6 * (size_t)e;
    mv6(u, d.A + 36 * (size_t)e, false, p + 6 * (size_t)d.ij[2 * e], 1.0, false);          // (p is zero at a fixed node)
    mv6(u, d.B + 36 * (size_t)e, false, p + 6 * (size_t)d.ij[2 * e + 1], 1.0, true);
  }
  c.sync();
  for (int k = c.tid(); k < d.n; k += c.nthreads()) {
    double t[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (!d.fixed[k]) {
      for (int at = d.csr_off[k]; at < d.csr_off[k + 1]; ++at) {
        const int e = d.csr_edge[at];
        mv6(t, (d.ij[2 * e] == k ? d.A : d.B) + 36 * (size_t)e, true, d.u + 6 * (size_t)e, 1.0, true);
      }
      if (lambda != 0.0) mv6(t, d.Hkk + 36 * (size_t)k, false, p + 6 * (size_t)k, lambda, true);
    }
    for (int a = 0; a < 6; ++a) q[6 * (size_t)k + a] = t[a];
  }
  c.sync();
}

template <class Ctx>
PG_HD double dot(const Dev& d, Ctx& c, const double* a, const double* b) {
  double s = 0.0;
  for (int k = c.tid(); k < d.n; k += c.nthreads())
    for (int t = 0; t < 6; ++t) s += a[6 * (size_t)k + t] * b[6 * (size_t)k + t];
  return c.sum(s);
}

// (H + lambda blockdiag(H)) x = -g from x = 0; the iterations
template <class Ctx>
PG_HD int pcg(const Dev& d, Ctx& c, double lambda, int cap, double tol = kPcgTol) {
  for (int k = c.tid(); k < 6 * d.n; k += c.nthreads()) { d.r[k] = -d.g[k]; d.x[k] = 0.0; }
  c.sync();
  apply_minv(d, c, d.r, d.z);
  for (int k = c.tid(); k < 6 * d.n; k += c.nthreads()) d.p[k] = d.z[k];
  double rz = dot(d, c, d.r, d.z);                                      // (its barriers publish p)
  const double rz0 = rz;
  if (!(rz0 > 0.0)) return 0;
  int it = 0;
  while (it < cap) {
    hmul(d, c, lambda, d.p, d.q);
    const double pq = dot(d, c, d.p, d.q);
    if (!(pq > 0.0)) break;
    const double al = rz / pq;
    for (int k = c.tid(); k < 6 * d.n; k += c.nthreads()) { d.x[k] += al * d.p[k]; d.r[k] -= al * d.q[k]; }
    c.sync();
    ++it;
    apply_minv(d, c, d.r, d.z);
    const double rz1 = dot(d, c, d.r, d.z);
    if (!(rz1 > tol * tol * rz0)) break;
    const double beta = rz1 / rz;
    for (int k = c.tid(); k < 6 * d.n; k += c.nthreads()) d.p[k] = d.z[k] + beta * d.p[k];
    c.sync();
    rz = rz1;
  }
  return it;
}

template <class Ctx>
PG_HD void retract_all(const Dev& d, Ctx& c, const double* X, double* Y) {
  for (int k = c.tid(); k < d.n; k += c.nthreads()) {
    const double* a = X + 12 * (size_t)k;
    double* o = Y + 12 * (size_t)k;
    if (d.fixed[k]) { for (int t = 0; t < 12; ++t) o[t] = a[t]; continue; }
    const double* dx = d.x + 6 * (size_t)k;
    double E[9];
    exp_so3(dx, E);
    for (int r = 0; r < 3; ++r) {
      for (int cc = 0; cc < 3; ++cc) o[3 * r + cc] = a[3 * r] * E[cc] + a[3 * r + 1] * E[3 + cc] + a[3 * r + 2] * E[6 + cc];
      o[9 + r] = a[9 + r] + (a[3 * r] * dx[3] + a[3 * r + 1] * dx[4] + a[3 * r + 2] * dx[5]);
    }
  }
  c.sync();
}

// The whole optimisation; the result is left in d.cur.
template <class Ctx>
PG_HD void run(const Dev& d, Ctx& c) {
  double* cur = d.cur;
  double* cand = d.cand;
  if (d.probe == 2) {                                                        // one thread, one factor; cur is only read
    for (int e = c.tid(); e < d.m; e += c.nthreads()) {
      const double s2 = edge_norm2(d, cur, e);
      d.rep_s[e] = sqrt(s2); d.wgt[e] = huber_weight(d, e, s2); d.rep_c[e] = huber_term(d, e, s2);
    }
    return;
  }
  if (d.probe) {                                                             // 1: at pose0 itself (cur keeps the last loop's result for the report)
    linearize(d, c, d.probe == 3 ? cur : d.pose0);                           // 3: at cur, which is only read
    assemble(d, c);
    const bool ok = factor(d, c, 0.0);
    if (d.probe == 3) {                                                      // ... and nothing else; a pivot that is not positive: NUMERIC
      if (c.tid() == 0) d.out_i[kOutStop] = ok ? 0 : SMHIP_POSE_GRAPH_STOP_NUMERIC;
      return;
    }
    for (int k = c.tid(); k < 6 * d.n; k += c.nthreads()) d.r[k] = d.fixed[k / 6] ? 0.0 : d.v[k];
    c.sync();
    apply_minv(d, c, d.r, d.minv);
    return;
  }
  for (int k = c.tid(); k < 12 * d.n; k += c.nthreads()) cur[k] = d.pose0[k];
  c.sync();
  double c0 = total_cost(d, c, cur);
  const double initial = c0;
  double lambda = 0.0;
  bool fresh = true;
  int stop = SMHIP_POSE_GRAPH_STOP_MAX_ITERATIONS, it = 0, accepted = 0, rejected = 0, pcg_total = 0, pcg_max = 0;
  if (!(c0 < 1.0e300)) stop = SMHIP_POSE_GRAPH_STOP_NUMERIC;
  while (stop == SMHIP_POSE_GRAPH_STOP_MAX_ITERATIONS && it < d.max_it) {
    if (fresh) { linearize(d, c, cur); assemble(d, c); fresh = false; }
    if (!factor(d, c, lambda)) { stop = SMHIP_POSE_GRAPH_STOP_NUMERIC; break; }
    const int left = d.pcg_budget - pcg_total;                            // the launch's own bound, beside the per-solve cap
    if (left <= 0) break;                                                 // (MAX_ITERATIONS)
    const int its = pcg(d, c, lambda, left < d.pcg_cap ? left : d.pcg_cap);
    pcg_total += its;
    pcg_max = its > pcg_max ? its : pcg_max;
    ++it;
    double big = 0.0;
    for (int k = c.tid(); k < 6 * d.n; k += c.nthreads()) big = fmax(big, fabs(d.x[k]));
    big = c.max(big);
    retract_all(d, c, cur, cand);
    const double c1 = total_cost(d, c, cand);
    if (!(c1 < 1.0e300) || !(big < 1.0e300)) { stop = SMHIP_POSE_GRAPH_STOP_NUMERIC; break; }
    if (big < kStepTol) {
      double* t = cur; cur = cand; cand = t;
      c0 = c1; ++accepted;
      stop = SMHIP_POSE_GRAPH_STOP_STEP;
    } else if (c1 <= c0 + (kCostTol * c0 + kCostNoise * sqrt(c0))) {      // within the rounding of the cost counts as "not raised"
      const double was = c0, band = kCostTol * c0 + kCostNoise * sqrt(c0);
      double* t = cur; cur = cand; cand = t;
      c0 = c1; ++accepted; fresh = true;
      lambda = lambda <= kLambdaFirst ? 0.0 : lambda / 10.0;
      if (was - c1 <= band) stop = SMHIP_POSE_GRAPH_STOP_COST;       // ... and a decrease inside it as none
    } else {
      ++rejected;
      lambda = lambda == 0.0 ? kLambdaFirst : 10.0 * lambda;
      if (lambda > kLambdaMax) stop = SMHIP_POSE_GRAPH_STOP_DAMPING;
    }
  }
  if (cur != d.cur) {
    for (int k = c.tid(); k < 12 * d.n; k += c.nthreads()) d.cur[k] = cur[k];
  }
  if (c.tid() == 0) {
    d.out_d[kOutInitial] = initial; d.out_d[kOutFinal] = c0; d.out_d[kOutLambda] = lambda;
    d.out_i[kOutStop] = stop; d.out_i[kOutIterations] = it; d.out_i[kOutAccepted] = accepted; d.out_i[kOutRejected] = rejected;
    d.out_i[kOutPcg] = pcg_total; d.out_i[kOutPcgMax] = pcg_max;
  }
}

// ---- marginal covariances ("Marginal covariances"; tests/pose_graph_marginals_ref.py) -------------------------
//
// After run() with probe = 3 the shared arrays A, B, Hkk, Dinv, Wm, Wp hold H = sum w J^T J at cur and the factors of its
// block-tridiagonal part M at lambda = 0; from then on they are only read.  Column c of node k of H^-1 solves H x = e_{6k+c}: the
// optimiser's own pcg from x = 0 with g = -e_{6k+c}, stopped at kMarginalPcgTol or the cap.  A workgroup (or the one host thread)
// works through a copy of Dev whose x r z p q b g u point into its own slice of a workspace, so workgroups share nothing they write.

// d's vectors <- the slice at w: kMargNodeDoubles * n + kMargEdgeDoubles * m doubles
PG_HD void marginal_slice(Dev* d, double* w) {
  const size_t n6 = 6 * (size_t)d->n;
  d->x = w; d->r = w + n6; d->z = w + 2 * n6; d->p = w + 3 * n6; d->q = w + 4 * n6; d->b = w + 5 * n6; d->g = w + 6 * n6; d->u = w + 7 * n6;
}

// One query: cov (36, row-major) = (X + X^T) / 2 with X = [H^-1]_kk; blocks (36 per row node, may be nullptr with n_rows 0) =
// [H^-1]_{r,k}, unsymmetrised; info (kMargInts).  A fixed query node, and a fixed row node, give zeros.  The same bits whichever
// workgroup runs it and whatever was queried before: everything it reads of its slice it has written itself.
template <class Ctx>
PG_HD void marginal_query(const Dev& d, Ctx& c, int k, int n_rows, const int32_t* rows, double* cov, double* blocks, int32_t* info) {
  int total = 0, longest = 0, capped = 0;
  if (d.fixed[k]) {
    for (int a = c.tid(); a < 36; a += c.nthreads()) cov[a] = 0.0;
    for (long long a = c.tid(); a < 36LL * n_rows; a += c.nthreads()) blocks[a] = 0.0;
  } else {
    for (int t = c.tid(); t < 6 * d.n; t += c.nthreads()) d.g[t] = 0.0;
    c.sync();
    for (int col = 0; col < 6; ++col) {
      if (c.tid() == 0) d.g[6 * (size_t)k + col] = -1.0;
      c.sync();
      const int its = pcg(d, c, 0.0, d.pcg_cap, kMarginalPcgTol);
      total += its;
      longest = its > longest ? its : longest;
      {   // Did the solve end because the stop rule was met?  pcg also leaves at the cap, on r0^T M^-1 r0 or p^T H p not positive (a
          // singular H, a NaN in A or B), and says only how many iterations it ran; r and z are its last, so the rule is taken again:
          // the same sums with the same bits.  Anything else -- a NaN included -- raises the flag.
        const double rz_end = dot(d, c, d.r, d.z);
        for (int t = c.tid(); t < 6 * d.n; t += c.nthreads()) d.q[t] = -d.g[t];
        c.sync();
        apply_minv(d, c, d.q, d.p);
        const double rz0 = dot(d, c, d.q, d.p);
        if (!(rz0 > 0.0) || !(rz_end <= kMarginalPcgTol * kMarginalPcgTol * rz0)) capped = 1;
      }
      for (int a = c.tid(); a < 6; a += c.nthreads()) cov[6 * a + col] = d.x[6 * (size_t)k + a];
      for (int t = c.tid(); t < 6 * n_rows; t += c.nthreads()) {
        const int r = rows[t / 6], a = t % 6;
        blocks[36 * (size_t)(t / 6) + 6 * a + col] = d.fixed[r] ? 0.0 : d.x[6 * (size_t)r + a];
      }
      if (c.tid() == 0) d.g[6 * (size_t)k + col] = 0.0;
      c.sync();
    }
    if (c.tid() == 0)
      for (int a = 0; a < 6; ++a)
        for (int b = a + 1; b < 6; ++b) { const double s = 0.5 * (cov[6 * a + b] + cov[6 * b + a]); cov[6 * a + b] = s; cov[6 * b + a] = s; }
  }
  if (c.tid() == 0) { info[kMargPcg] = total; info[kMargPcgMax] = longest; info[kMargCapped] = capped; }
  c.sync();
}

// queries first, first + stride, ... of the call: what one workgroup of `stride` does
template <class Ctx>
PG_HD void marginal_queries(const Dev& d, Ctx& c, int first, int stride, int n_query, const int32_t* query, int n_rows, const int32_t* rows, double* cov,
                            double* blocks, int32_t* info) {
  for (long long q = first; q < n_query; q += stride)
    marginal_query(d, c, query[q], n_rows, rows, cov + 36 * (size_t)q, blocks ? blocks + 36 * (size_t)n_rows * (size_t)q : nullptr, info + kMargInts * (size_t)q);
}

}  // namespace pose_graph
}  // namespace smhip
