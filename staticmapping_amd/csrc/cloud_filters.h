// cloud_filters.h -- internal interface of the device-side pre-filters (cloud_filters.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cmath>
#include <cstdint>

struct smhip_filter_desc_ex;

namespace smhip {
struct FilterWorkspace;
FilterWorkspace* filt_create(int max_points);
void filt_destroy(FilterWorkspace* w);
// staged_dev: n device rows (x, y, z, intensity); factor: host array of n floats or NULL (= i / n, the collector's rule)
hipError_t filt_set_input(FilterWorkspace* w, hipStream_t st, const float4* staged_dev, const float* factor_host_or_null, int n);
// applies the filters in order to the current cloud; blocks until the size is known.  The descriptors are already valid
// (smhip_filter_config_valid_ex); the ground filters' device tables grow here on first use.
hipError_t filt_run_chain(FilterWorkspace* w, hipStream_t st, const smhip_filter_desc_ex* chain, int nf, int* n_out);
// A cloud that a kernel of another unit writes straight into the workspace (smhip_submap.hip).  filt_build_begin hands out the
// arrays of half 0 (room for the workspace's capacity) and clears *bad; the producer's kernel on `st` fills pts / fac / src and,
// for a VoxelGrid to follow, keys / idx (voxel_key.h; *bad = 1 when a key is out of range).  filt_build_commit makes the n rows
// the current cloud, runs the VoxelGrid from its sort on when `keyed`, and blocks until the size is known.  An out-of-range key
// returns hipErrorInvalidValue with the unfiltered rows as the current cloud, as a VoxelGrid in a chain leaves it.
struct FilterBuild { float4* pts; float* fac; int32_t* src; unsigned long long* keys; int32_t* idx; int32_t* bad; };
FilterBuild filt_build_begin(FilterWorkspace* w, hipStream_t st);
hipError_t filt_build_commit(FilterWorkspace* w, hipStream_t st, int n, bool keyed, int* n_out);
const float4* filt_points(const FilterWorkspace* w);         // x y z intensity
const float* filt_factors(const FilterWorkspace* w);
const int32_t* filt_source_index(const FilterWorkspace* w);  // row of the ORIGINAL input each point came from (-1 after VoxelGrid)
int filt_count(const FilterWorkspace* w);
bool filt_has_index(const FilterWorkspace* w);
// a warning the last filt_run_chain left ("" = none): a condition that is no error, for the handle's last-error text
const char* filt_note(const FilterWorkspace* w);
// the last StatisticRemoval of the last filt_run_chain: the rows it saw (-1: none ran, -2: it kept every row because no more than
// point_num_meank of them were finite), and on the device its distance[] in that row order and sum, sq_sum, V, threshold
int filt_statistic_rows(const FilterWorkspace* w);
const float* filt_statistic_distance(const FilterWorkspace* w);
const double* filt_statistic_stats(const FilterWorkspace* w);

// MotionCompensation (builder/map_builder.cc:232-257) of the current cloud, motion_comp.hip.  What InterpolateTransform
// (common/math.h:199-211) derives from delta alone, once per call: q_b = Eigen's Quaternion(Matrix3) of delta's rotation block
// (trace branch / largest-diagonal branch, w may come out negative in the second), d = q_a . q_b = q_b.w for q_a = (1, 0, 0, 0),
// the branch of Eigen's slerp (|d| >= 1 - DBL_EPSILON: linear scales), theta = acos(|d|), sin(theta), and whether the second
// scale is negated (d < 0).
struct MotionCompArgs {
  double bx, by, bz, bw;        // q_b
  double theta, sin_theta;      // unused when `linear`
  double tx, ty, tz;            // delta's translation
  int32_t linear, negate;
};
inline MotionCompArgs motion_comp_args(const double m[16] /* column-major 4x4 */) {
  auto R = [&](int r, int c) { return m[4 * c + r]; };
  MotionCompArgs a{};
  double q[3], w, t = R(0, 0) + R(1, 1) + R(2, 2);
  if (t > 0) {
    t = std::sqrt(t + 1.0); w = 0.5 * t; t = 0.5 / t;
    q[0] = (R(2, 1) - R(1, 2)) * t; q[1] = (R(0, 2) - R(2, 0)) * t; q[2] = (R(1, 0) - R(0, 1)) * t;
  } else {
    int i = 0; if (R(1, 1) > R(0, 0)) i = 1; if (R(2, 2) > R(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0); q[i] = 0.5 * t; t = 0.5 / t;
    w = (R(k, j) - R(j, k)) * t; q[j] = (R(j, i) + R(i, j)) * t; q[k] = (R(k, i) + R(i, k)) * t;
  }
  a.bx = q[0]; a.by = q[1]; a.bz = q[2]; a.bw = w;
  const double d = 1.0 * w + 0.0 * q[0] + 0.0 * q[1] + 0.0 * q[2], abs_d = std::fabs(d);
  a.linear = abs_d >= 1.0 - 2.220446049250313e-16 ? 1 : 0;
  if (!a.linear) { a.theta = std::acos(abs_d); a.sin_theta = std::sin(a.theta); }
  a.negate = d < 0 ? 1 : 0;
  a.tx = m[12]; a.ty = m[13]; a.tz = m[14];
  return a;
}
// writes the compensated rows (x y z intensity, the workspace's row order) to `out` (room for filt_count rows) and leaves the
// workspace as it was.  A row whose factor is outside [0, 1] or NaN sets a device flag by a plain store (the row is copied
// unchanged); the flag travels to pinned memory behind the kernel: once `st` has been synchronised, filt_motion_bad_factor says
// whether the last call met such a row.  Asynchronous on `st`.
hipError_t filt_motion_compensate(FilterWorkspace* w, hipStream_t st, const MotionCompArgs& a, float4* out);
bool filt_motion_bad_factor(const FilterWorkspace* w);
// The same flag for a kernel of another unit that de-skews the rows it builds (smhip_submap.hip, between filt_build_begin and
// filt_build_commit): filt_motion_flag_begin clears it on `st` and hands it out (nullptr: the clear failed), the kernel raises it by
// a plain store, filt_motion_flag_end sends it to pinned memory behind the kernel; filt_motion_bad_factor reads it once `st` has been
// synchronised.
int32_t* filt_motion_flag_begin(FilterWorkspace* w, hipStream_t st);
hipError_t filt_motion_flag_end(FilterWorkspace* w, hipStream_t st);

// GroundRemoval2::ClusterGround, filter_ground_removal2.cc:318-320: search_angle_ / 180. * M_PI / delta_alpha in double with
// delta_alpha = (float)(M_PI * 2 / segment_num_), truncated as x86 does (INT_MIN outside the int range)
inline int gr2_search_step(float search_angle, int segment_num) {
  const float delta_alpha = M_PI * 2 / segment_num;
  const double v = search_angle / 180. * M_PI / delta_alpha;
  return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN;
}
}  // namespace smhip
