// motion_comp.hip -- the front end's MotionCompensation on the device (included by cloud_filters.hip, inside its namespace).
//
// Reference: MotionCompensation, builder/map_builder.cc:232-257 -- for every row, with f = point.factor,
//     transform = common::InterpolateTransform(I, delta, f)             common/math.h:199-211
//     new point = Rotation(transform) * Vector3d(x, y, z) + Translation(transform), each coordinate cast to float
// InterpolateTransform is Eigen's q_a.slerp(f, q_b).toRotationMatrix() with q_a = (1, 0, 0, 0), q_b = Quaternion(delta's
// rotation block), and the translation delta.t * (double)f.  What depends on delta alone -- q_b, d = q_a . q_b = q_b.w, the
// branch of the slerp, theta = acos(|d|), sin(theta), the sign of the second scale -- is computed once on the host
// (MotionCompArgs, cloud_filters.h); the kernel evaluates per row what depends on the factor: the two scales, the interpolated
// quaternion (NOT normalised, as in Eigen), Eigen's toRotationMatrix terms and the product, all in double and operation by
// operation (no fused multiply-add: the reference builds without it).
//
// One thread per row, 256-thread blocks: a 16-byte load of the row, a 4-byte load of its factor, a 16-byte store.  A factor
// outside [0, 1] or NaN (CHECK(factor >= 0. && factor <= 1.), math.h:202) raises *bad by a plain store; the row is copied as it is.

__global__ __launch_bounds__(256) void filt_motion_comp(const float4* __restrict__ pts, const float* __restrict__ fac, int n,
                                                        MotionCompArgs a, float4* __restrict__ out, int32_t* __restrict__ bad) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  const float f = fac[i];
  if (!((double)f >= 0. && (double)f <= 1.)) { bad[0] = 1; out[i] = p; return; }
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
  const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
  const double nx = ((r00 * x + r01 * y) + r02 * z) + a.tx * t;           // map_builder.cc:244-247
  const double ny = ((r10 * x + r11 * y) + r12 * z) + a.ty * t;
  const double nz = ((r20 * x + r21 * y) + r22 * z) + a.tz * t;
  out[i] = make_float4((float)nx, (float)ny, (float)nz, p.w);              // :250-253 (intensity carried; the factor stays where it is)
}
