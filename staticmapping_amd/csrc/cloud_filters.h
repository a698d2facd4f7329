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
const float4* filt_points(const FilterWorkspace* w);         // x y z intensity
const float* filt_factors(const FilterWorkspace* w);
const int32_t* filt_source_index(const FilterWorkspace* w);  // row of the ORIGINAL input each point came from (-1 after VoxelGrid)
int filt_count(const FilterWorkspace* w);
bool filt_has_index(const FilterWorkspace* w);

// GroundRemoval2::ClusterGround, filter_ground_removal2.cc:318-320: search_angle_ / 180. * M_PI / delta_alpha in double with
// delta_alpha = (float)(M_PI * 2 / segment_num_), truncated as x86 does (INT_MIN outside the int range)
inline int gr2_search_step(float search_angle, int segment_num) {
  const float delta_alpha = M_PI * 2 / segment_num;
  const double v = search_angle / 180. * M_PI / delta_alpha;
  return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN;
}
}  // namespace smhip
