// icp_tail_math.h -- the pure arithmetic of the serial end of an IcpFast iteration (finalize_tail, icp_kernels.hip): the 6x6 solve
// with its invertibility rule, the angle-axis step with its NaN guard, the motion-potential bound, Eigen's quaternion of a
// rotation, angularDistance and CheckConvergence over the history ring (registrators/icp_fast.cc:204-254, 306-323, 377-405).
//
// It stands in a header so that two compilers read the same text: hipcc for the kernels (`finalize`, `finalize_comp`, the
// one-launch kernel of icp_one.hip) and g++ -D__HIP_PLATFORM_AMD__ for tests/cpp/test_icp_tail.cc, which runs every branch of it
// against a multi-precision reference without a device.  No state, no HIP runtime call: plain doubles in, plain doubles out.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace smhip {

__host__ __device__ inline __noinline__ void jacobi_eig6(double* A, double* V, double* w) {
  for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) V[6 * i + j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
    for (int i = 0; i < 6; ++i) for (int j = i + 1; j < 6; ++j) off += A[6 * i + j] * A[6 * i + j];
    if (off < 1e-300) break;
    for (int p = 0; p < 6; ++p)
      for (int q = p + 1; q < 6; ++q) {
        const double apq = A[6 * p + q];
        if (fabs(apq) < 1e-300) continue;
        const double theta = (A[6 * q + q] - A[6 * p + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 6; ++k) { const double akp = A[6 * k + p], akq = A[6 * k + q]; A[6 * k + p] = c * akp - s * akq; A[6 * k + q] = s * akp + c * akq; }
        for (int k = 0; k < 6; ++k) { const double apk = A[6 * p + k], aqk = A[6 * q + k]; A[6 * p + k] = c * apk - s * aqk; A[6 * q + k] = s * apk + c * aqk; }
        for (int k = 0; k < 6; ++k) { const double vkp = V[6 * k + p], vkq = V[6 * k + q]; V[6 * k + p] = c * vkp - s * vkq; V[6 * k + q] = s * vkp + c * vkq; }
      }
  }
  for (int i = 0; i < 6; ++i) w[i] = A[6 * i + i];
}

// fullPivHouseholderQr().rank() of a 6x6 (Eigen/src/QR/FullPivHouseholderQR.h): the pivots |R_kk| of the Householder QR that
// brings the largest remaining entry to the corner at every step, counted above eps * 6 * (largest pivot); the elimination stops
// at a corner whose largest entry is below eps * 6 (Eigen's m_precision) times the first corner's; the pivots after it are zero.  isInvertible() is
// rank == 6.  Only the slow path of solve6 calls it.
// M is destroyed and piv[6] is scratch: the caller lends what jacobi_eig6 will use afterwards, so the slow path needs no more stack.
__host__ __device__ inline __noinline__ int qr_rank6(double* M, double* piv) {
  const double kPrec = 2.220446049250313e-16 * 6;
  for (int i = 0; i < 36; ++i) if (!isfinite(M[i])) return 0;
  for (int k = 0; k < 6; ++k) piv[k] = 0;
  double maxpivot = 0, biggest = 0;
  for (int k = 0; k < 6; ++k) {
    int pr = k, pc = k;
    double big = -1;
    for (int i = k; i < 6; ++i)
      for (int j = k; j < 6; ++j) if (fabs(M[6 * i + j]) > big) { big = fabs(M[6 * i + j]); pr = i; pc = j; }
    if (k == 0) biggest = big;
    if (!(big > biggest * kPrec)) break;                    // isMuchSmallerThan(biggest_in_corner, biggest, m_precision)
    for (int j = 0; j < 6; ++j) { const double t = M[6 * k + j]; M[6 * k + j] = M[6 * pr + j]; M[6 * pr + j] = t; }
    for (int i = 0; i < 6; ++i) { const double t = M[6 * i + k]; M[6 * i + k] = M[6 * i + pc]; M[6 * i + pc] = t; }
    double tail2 = 0;                                       // makeHouseholder of column k below the diagonal
    for (int i = k + 1; i < 6; ++i) tail2 += M[6 * i + k] * M[6 * i + k];
    const double c0 = M[6 * k + k];
    double beta = c0;
    if (tail2 > 0) {
      beta = sqrt(c0 * c0 + tail2);
      if (c0 >= 0) beta = -beta;
      const double den = c0 - beta, tau = (beta - c0) / beta;
      for (int j = k + 1; j < 6; ++j) {                    // (I - tau v v^T) applied to the trailing columns, v = (1, tail / den)
        double s = M[6 * k + j];
        for (int i = k + 1; i < 6; ++i) s += (M[6 * i + k] / den) * M[6 * i + j];
        s *= tau;
        M[6 * k + j] -= s;
        for (int i = k + 1; i < 6; ++i) M[6 * i + j] -= s * (M[6 * i + k] / den);
      }
    }
    piv[k] = fabs(beta);
    maxpivot = fmax(maxpivot, piv[k]);
  }
  int rank = 0;
  for (int k = 0; k < 6; ++k) rank += (piv[k] > kPrec * maxpivot) ? 1 : 0;
  return rank;
}

// which way solve6 went: what tests/cpp/test_icp_tail.cc records beside x
enum Solve6Branch : int {
  kSolveCholeskyFast = 0,   // every Cholesky pivot cleared kSolveFastAccept * dmax: no other decision is taken
  kSolveCholeskyQr = 1,     // a pivot did not, the full-pivot QR reports rank 6: Cholesky all the same
  kSolveMinNorm = 2,        // the QR reports rank < 6 (or Cholesky broke down): minimum-norm solution of that rank
};

// The fast accept: every pivot of the unpivoted Cholesky above kSolveFastAccept * dmax (dmax = the largest diagonal entry).
// The multiple has to stand above the factorisation's own rounding: a pivot is a difference whose error grows with
// 1 / (the smallest pivot before it), about eps * dmax / multiple, so a multiple m is only trustworthy while m >> eps / m, i.e.
// m >> 1.5e-8.  The 1e-13 this code once used was not: on a matrix with lambda_min / lambda_max = 1e-17 and middle eigenvalues at
// 1e-3 the computed last pivot is 2e-13 dmax of pure rounding, the accept took it for invertible and Cholesky solved a singular
// system (decision ladder of tests/test_icp_tail_cpp.py, rung full:1e-17:dense).  At 1e-6 the pivots are good to 1e-9 of dmax and
// the ladder shows no accepted matrix within ten times the reference's threshold; scans sit at 1e-3 and above (a 20 000-point
// synthetic pair: smallest pivot 1.8e-3 dmax), so ordinary iterations never leave the fast path.
constexpr double kSolveFastAccept = 1e-6;

// L y = rhs, L^T x = y, unrolled like the factorisation
__host__ __device__ __forceinline__ void solve6_substitute(const double* L, const double* rhs, double* x) {
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = rhs[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[6 * i + k] * y[k];
    y[i] = s / L[6 * i + i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[6 * k + i] * x[k];
    x[i] = s / L[6 * i + i];
  }
}

// SolvePossiblyUnderdeterminedLinearSystem (icp_fast.cc:204-254): Cholesky when A is invertible by the reference's rule --
// fullPivHouseholderQr().isInvertible(), every QR pivot above eps * 6 * the largest --, otherwise the minimum-norm solution of the
// system reduced to the rank that QR reports (pseudo-inverse over the `rank` largest eigenvalues).
__host__ __device__ __forceinline__ int solve6(const double* A, const double* rhs, double* x) {
  // fully unrolled so that L lives in registers: with run-time indices it sits in scratch memory and every access is a
  // memory round trip (the serial tail of finalize took 9-19 us that way)
  double L[36];
  double dmax = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) dmax = fmax(dmax, fabs(A[6 * i + i]));
  bool ok = dmax > 0 && isfinite(dmax);
  bool pos = ok;                                            // every pivot > 0: the factor exists
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = A[6 * i + j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[6 * i + k] * L[6 * j + k];
      if (i == j) {
        ok = ok && (s > kSolveFastAccept * dmax);
        pos = pos && (s > 0);
        L[6 * i + i] = sqrt(s);
      } else {
        L[6 * i + j] = s / L[6 * j + j];
      }
    }
  double E[36], V[36], w[6];
  int branch = kSolveCholeskyFast, rank = 6;
  if (!ok) {                                                // the slow path: the reference's own rule decides
#pragma unroll
    for (int i = 0; i < 36; ++i) E[i] = A[i];
    rank = qr_rank6(E, w);
    ok = pos && rank == 6;
    branch = ok ? kSolveCholeskyQr : kSolveMinNorm;
  }
  if (ok) {
    solve6_substitute(L, rhs, x);
    return branch;
  }
#pragma unroll
  for (int i = 0; i < 36; ++i) E[i] = A[i];
  jacobi_eig6(E, V, w);
  // the `rank` largest |eigenvalues| are kept (rank 6 here means Cholesky broke down on a matrix the QR calls invertible: all
  // six); a non-finite A has rank 0 by qr_rank6 and x = 0
  unsigned keep = 0;
  for (int n = 0; n < rank; ++n) {
    int best = -1;
    double wbest = 0;
    for (int k = 0; k < 6; ++k) if (!((keep >> k) & 1u) && fabs(w[k]) > wbest) { best = k; wbest = fabs(w[k]); }
    if (best < 0) break;
    keep |= 1u << best;
  }
  for (int i = 0; i < 6; ++i) x[i] = 0;
  for (int k = 0; k < 6; ++k) {
    if (!((keep >> k) & 1u)) continue;
    double c = 0;
    for (int i = 0; i < 6; ++i) c += V[6 * i + k] * rhs[i];
    c /= w[k];
    for (int i = 0; i < 6; ++i) x[i] += c * V[6 * i + k];
  }
  return kSolveMinNorm;
}

__host__ __device__ __forceinline__ void quat_from_rot(const double* T, double* q) {   // Eigen::Quaterniond(Matrix3d), T row-major 4x4
  const double r00 = T[0], r01 = T[1], r02 = T[2], r10 = T[4], r11 = T[5], r12 = T[6], r20 = T[8], r21 = T[9], r22 = T[10];
  const double tr = r00 + r11 + r22;
  if (tr > 0) {
    const double s = sqrt(tr + 1.0) * 2;
    q[0] = 0.25 * s; q[1] = (r21 - r12) / s; q[2] = (r02 - r20) / s; q[3] = (r10 - r01) / s;
  } else if (r00 >= r11 && r00 >= r22) {
    const double s = sqrt(1.0 + r00 - r11 - r22) * 2;
    q[0] = (r21 - r12) / s; q[1] = 0.25 * s; q[2] = (r01 + r10) / s; q[3] = (r02 + r20) / s;
  } else if (r11 >= r22) {
    const double s = sqrt(1.0 + r11 - r00 - r22) * 2;
    q[0] = (r02 - r20) / s; q[1] = (r01 + r10) / s; q[2] = 0.25 * s; q[3] = (r12 + r21) / s;
  } else {
    const double s = sqrt(1.0 + r22 - r00 - r11) * 2;
    q[0] = (r10 - r01) / s; q[1] = (r02 + r20) / s; q[2] = (r12 + r21) / s; q[3] = 0.25 * s;
  }
}

__host__ __device__ __forceinline__ double quat_angular_distance(const double* a, const double* c) {
  const double w = a[0] * c[0] + a[1] * c[1] + a[2] * c[2] + a[3] * c[3];
  const double x = -a[0] * c[1] + a[1] * c[0] - a[2] * c[3] + a[3] * c[2];
  const double y = -a[0] * c[2] + a[2] * c[0] - a[3] * c[1] + a[1] * c[3];
  const double z = -a[0] * c[3] + a[3] * c[0] - a[1] * c[2] + a[2] * c[1];
  return 2.0 * atan2(sqrt(x * x + y * y + z * z), fabs(w));
}

// transform = AngleAxis(|x[0:3]|, x[0:3] / |x[0:3]|), translation = x[3:6]    :306-312; a NaN anywhere in it resets the rotation
// block to the identity and keeps the translation (:315-321).  dT is a row-major 4x4 whose last row the caller has set.
__host__ __device__ __forceinline__ void angle_axis_step(const double* x, double* dT) {
  const double ang = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const double ax = x[0] / ang, ay = x[1] / ang, az = x[2] / ang;
  const double c = cos(ang), s = sin(ang), v = 1.0 - c;
  double R[9] = {c + v * ax * ax, v * ax * ay - s * az, v * ax * az + s * ay,
                 v * ax * ay + s * az, c + v * ay * ay, v * ay * az - s * ax,
                 v * ax * az - s * ay, v * ay * az + s * ax, c + v * az * az};
  bool has_nan = false;
  for (int i = 0; i < 9; ++i) has_nan |= isnan(R[i]);
  for (int i = 0; i < 3; ++i) has_nan |= isnan(x[3 + i]);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) dT[4 * i + j] = has_nan ? ((i == j) ? 1.0 : 0.0) : R[3 * i + j];   // :315-321
  dT[3] = x[3]; dT[7] = x[4]; dT[11] = x[5];
}

// motion potential: this step's ||dR|| and |dt| (what bounds |M_new s - M_old s| <= ||dR|| |s| + |dt|).
// ||dR|| is the SPECTRAL norm of the 3x3 difference (the largest singular value: what |dR s| <= ||dR|| |s| needs), from the
// closed-form largest eigenvalue of dR^T dR with 1e-6 of slack and never more than the Frobenius norm; for the difference of
// two rotations the Frobenius norm is sqrt(2) times larger, and with it sqrt(2) times the certified motion of far points.
// Mn, M: row-major 3x4 (or 4x4) poses.
__host__ __device__ __forceinline__ void motion_potential_step(const double* Mn, const double* M, double* step_a, double* step_b) {
  double D[9], fa = 0, fb = 0;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) { D[3 * r + c] = Mn[4 * r + c] - M[4 * r + c]; fa += D[3 * r + c] * D[3 * r + c]; }
    const double d = Mn[4 * r + 3] - M[4 * r + 3];
    fb += d * d;
  }
  double S[6];                                           // D^T D: xx xy xz yy yz zz
  S[0] = D[0] * D[0] + D[3] * D[3] + D[6] * D[6]; S[1] = D[0] * D[1] + D[3] * D[4] + D[6] * D[7]; S[2] = D[0] * D[2] + D[3] * D[5] + D[6] * D[8];
  S[3] = D[1] * D[1] + D[4] * D[4] + D[7] * D[7]; S[4] = D[1] * D[2] + D[4] * D[5] + D[7] * D[8]; S[5] = D[2] * D[2] + D[5] * D[5] + D[8] * D[8];
  double lam = fa;                                       // trace = squared Frobenius norm >= the largest eigenvalue
  {
    const double q = (S[0] + S[3] + S[5]) / 3.0;
    const double p1 = S[1] * S[1] + S[2] * S[2] + S[4] * S[4];
    const double p2 = (S[0] - q) * (S[0] - q) + (S[3] - q) * (S[3] - q) + (S[5] - q) * (S[5] - q) + 2.0 * p1;
    if (p2 > 0.0 && isfinite(p2)) {
      const double p = sqrt(p2 / 6.0), ip = 1.0 / p;
      const double b0 = (S[0] - q) * ip, b3 = (S[3] - q) * ip, b5 = (S[5] - q) * ip, b1 = S[1] * ip, b2 = S[2] * ip, b4 = S[4] * ip;
      double r = 0.5 * (b0 * (b3 * b5 - b4 * b4) - b1 * (b1 * b5 - b4 * b2) + b2 * (b1 * b4 - b3 * b2));
      r = fmin(1.0, fmax(-1.0, r));
      const double est = (q + 2.0 * p * cos(acos(r) / 3.0)) * (1.0 + 2e-6) + 1e-300;
      if (isfinite(est) && est > 0.0) lam = fmin(lam, est);
    } else if (p2 == 0.0) {
      lam = fmin(lam, q * (1.0 + 2e-6));
    }
  }
  *step_a = sqrt(lam) * (1.0 + 1e-9); *step_b = sqrt(fb) * (1.0 + 1e-9);
}

// The history ring (latest at n_hist-1, at most 5 kept) takes the pose Tn, then CheckConvergence (:377-405, kSmoothLength = 4):
// with more than four entries, the means of the last four rotation and translation steps below 1e-3 rad and 1e-2 m.
__host__ __device__ __forceinline__ bool history_push_converged(double (*quat)[4], double (*trans)[3], int32_t* n_hist, const double* Tn,
                                                                bool early_exit) {
  int nh = *n_hist;
  if (nh == 5) {
    for (int k = 0; k < 4; ++k) {
      for (int c = 0; c < 4; ++c) quat[k][c] = quat[k + 1][c];
      for (int c = 0; c < 3; ++c) trans[k][c] = trans[k + 1][c];
    }
    nh = 4;
  }
  quat_from_rot(Tn, quat[nh]);
  trans[nh][0] = Tn[3]; trans[nh][1] = Tn[7]; trans[nh][2] = Tn[11];
  *n_hist = ++nh;
  bool converged = false;
  if (early_exit && nh > 4) {                                               // :377-405 (kSmoothLength = 4)
    double rd = 0, td = 0;
    for (int k = nh - 1; k >= nh - 4; --k) {
      rd += fabs(quat_angular_distance(quat[k], quat[k - 1]));
      const double dx = trans[k][0] - trans[k - 1][0], dy = trans[k][1] - trans[k - 1][1], dz = trans[k][2] - trans[k - 1][2];
      td += sqrt(dx * dx + dy * dy + dz * dz);
    }
    converged = (rd / 4 < 1e-3) && (td / 4 < 1e-2);
  }
  return converged;
}

}  // namespace smhip
