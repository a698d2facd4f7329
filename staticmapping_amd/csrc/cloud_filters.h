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

// GroundRemoval2::ClusterGround, filter_ground_removal2.cc:318-320: search_angle_ / 180. * M_PI / delta_alpha in double with
// delta_alpha = (float)(M_PI * 2 / segment_num_), truncated as x86 does (INT_MIN outside the int range)
inline int gr2_search_step(float search_angle, int segment_num) {
  const float delta_alpha = M_PI * 2 / segment_num;
  const double v = search_angle / 180. * M_PI / delta_alpha;
  return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN;
}
}  // namespace smhip
