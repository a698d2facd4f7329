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
// operation (no fused multiply-add: the reference builds without it) -- motion_comp_point (motion_comp_point.h), which the map's
// and the submap build's de-skewing kernels share.
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
  if (!motion_comp_factor_ok(f)) { bad[0] = 1; out[i] = p; return; }
  const float3 q = motion_comp_point(a, p.x, p.y, p.z, f);                 // motion_comp_point.h
  out[i] = make_float4(q.x, q.y, q.z, p.w);                                // :250-253 (intensity carried; the factor stays where it is)
}
