// motion_comp_point.h -- MotionCompensation of one row (builder/map_builder.cc:232-257), the arithmetic every de-skewing kernel of
// the library shares: filt_motion_comp (motion_comp.hip), mrvm_transform_comp (smhip_mrvm.hip) and submap_transform_keys_comp
// (smhip_submap.hip).  It stands once so that the three give the same bits.  Device code only; MotionCompArgs and what the host
// derives from delta alone are in cloud_filters.h.
#pragma once
#include <hip/hip_runtime.h>

#include "cloud_filters.h"

namespace smhip {

// CHECK(factor >= 0. && factor <= 1.), common/math.h:202 (a NaN fails both comparisons)
__device__ __forceinline__ bool motion_comp_factor_ok(float f) { return (double)f >= 0. && (double)f <= 1.; }

// InterpolateTransform(I, delta, f) applied to (x, y, z): what depends on the factor -- the two slerp scales, the interpolated
// quaternion (NOT normalised, as in Eigen), Eigen's toRotationMatrix terms and the product -- in double and operation by operation
// (no fused multiply-add: the reference builds without it), each coordinate then cast to float.  `f` has passed
// motion_comp_factor_ok.
__device__ __forceinline__ float3 motion_comp_point(const MotionCompArgs& a, float px, float py, float pz, float f) {
#pragma clang fp contract(off)
  const double t = (double)f;
  double scale0, scale1;                                                   // Eigen/src/Geometry/Quaternion.h, slerp
  if (a.linear) { scale0 = 1.0 - t; scale1 = t; }
  else { scale0 = sin((1.0 - t) * a.theta) / a.sin_theta; scale1 = sin(t * a.theta) / a.sin_theta; }
  if (a.negate) scale1 = -scale1;
  // scale0 * q_a.coeffs() + scale1 * q_b.coeffs() with q_a = (x 0, y 0, z 0, w 1)
  const double qx = scale0 * 0.0 + scale1 * a.bx, qy = scale0 * 0.0 + scale1 * a.by, qz = scale0 * 0.0 + scale1 * a.bz;
  const double qw = scale0 * 1.0 + scale1 * a.bw;
  const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;                // toRotationMatrix
  const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
  const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
  const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
  const double r00 = 1.0 - (tyy + tzz), r01 = txy - twz, r02 = txz + twy;
  const double r10 = txy + twz, r11 = 1.0 - (txx + tzz), r12 = tyz - twx;
  const double r20 = txz - twy, r21 = tyz + twx, r22 = 1.0 - (txx + tyy);
  const double x = (double)px, y = (double)py, z = (double)pz;
  const double nx = ((r00 * x + r01 * y) + r02 * z) + a.tx * t;           // map_builder.cc:244-247
  const double ny = ((r10 * x + r11 * y) + r12 * z) + a.ty * t;
  const double nz = ((r20 * x + r21 * y) + r22 * z) + a.tz * t;
  return make_float3((float)nx, (float)ny, (float)nz);                     // :250-253
}

}  // namespace smhip
