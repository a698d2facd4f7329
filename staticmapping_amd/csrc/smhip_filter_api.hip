// smhip_filter_api.hip -- C ABI of the device pre-filters: a translation unit of its own that launches no kernel (the kernels
// are in cloud_filters.hip, behind cloud_filters.h); the handle and check_slot / prep_ensure come from smhip_context.h.
// Mirrors pre_processers::filter::{Range, AxisRange, BoundingBoxRemoval, RandomSampler, VoxelGrid, GroundRemoval, GroundRemoval2,
// RangeImage, StatisticRemoval, Factory} (the reference's pre_processors/filter_*.cc): constructor defaults, ConfigsValid() and
// Filter().
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "smhip_context.h"

using namespace smhip_host;

namespace smhip_host {
smhip_status filter_ensure(smhip_context* h) {
  smhip_status s = prep_ensure(h);
  if (s) return s;
  if (h->filt) return SMHIP_OK;
  h->filt = filt_create(std::max(h->dev.ns_cap, h->dev.nt_cap));
  if (!h->filt) { h->err = "filter workspace allocation failed"; return SMHIP_ERR_HIP; }
  return SMHIP_OK;
}
}  // namespace smhip_host

extern "C" {

void smhip_filter_default(int type, smhip_filter_desc* f) {
  if (!f) return;
  std::memset(f, 0, sizeof(*f));
  f->type = type;
  switch (type) {
    case SMHIP_FILTER_RANGE: f->p[0] = 0.f; f->p[1] = FLT_MAX; break;                         // filter_range.cc:33-36
    case SMHIP_FILTER_AXIS_RANGE: f->p[0] = -FLT_MAX; f->p[1] = FLT_MAX; f->axis_index = 2; break;   // filter_axis_range.h:56-57, .cc:28
    case SMHIP_FILTER_RANDOM_SAMPLER: f->p[0] = 1.f; break;                                   // filter_random_sample.cc:28
    case SMHIP_FILTER_VOXEL_GRID: f->p[0] = 0.1f; break;                                      // filter_voxel_grid.h:55
    case SMHIP_FILTER_BOUNDING_BOX_REMOVAL:                                                   // filter_bounding_box.h:53-58
      f->p[0] = f->p[1] = f->p[2] = -FLT_MAX; f->p[3] = f->p[4] = f->p[5] = FLT_MAX; break;
    default: f->type = 0; break;
  }
}

int smhip_filter_config_valid(const smhip_filter_desc* f) {
  if (!f) return 0;
  switch (f->type) {
    case SMHIP_FILTER_RANGE: return 1;                                                        // no override: Interface default
    case SMHIP_FILTER_AXIS_RANGE: return (f->p[1] > f->p[0]) && f->axis_index >= 0 && f->axis_index <= 2;   // filter_axis_range.cc:40-42
    case SMHIP_FILTER_RANDOM_SAMPLER: return f->p[0] >= 0.f && f->p[0] <= 1.f;                 // filter_random_sample.cc:34-36
    case SMHIP_FILTER_VOXEL_GRID: return f->p[0] > 1.e-6;                                      // filter_voxel_grid.cc:36
    case SMHIP_FILTER_BOUNDING_BOX_REMOVAL: return f->p[0] < f->p[3] && f->p[1] < f->p[4] && f->p[2] < f->p[5];   // filter_bounding_box.cc:49-51
  }
  return 0;
}

static smhip_filter_desc_ex widen(const smhip_filter_desc& f) {
  smhip_filter_desc_ex e;
  std::memset(&e, 0, sizeof(e));
  e.type = f.type; e.seed = f.seed; e.i[0] = f.axis_index;
  for (int q = 0; q < 6; ++q) e.p[q] = f.p[q];
  return e;
}

constexpr long kMaxFilterCells = 1l << 22;        // GroundRemoval2 grids, RangeImage pixels
constexpr int kMaxBins = 4096;                    // GroundRemoval2: one segment's line points in LDS

// why the device cannot run the descriptor (nullptr = it can); the three new filters have no ConfigsValid() of their own
static const char* config_problem_ex(const smhip_filter_desc_ex* f) {
  if (!f) return "null descriptor";
  switch (f->type) {
    case SMHIP_FILTER_GROUND_REMOVAL:
      if (!(f->p[0] > 0.f) || !std::isfinite(f->p[0])) return "GroundRemoval: leaf_size must be a positive finite number";
      return nullptr;
    case SMHIP_FILTER_GROUND_REMOVAL2:
      if (f->i[0] <= 0 || f->i[1] <= 0) return "GroundRemoval2: bin_num and segment_num must be positive";
      if (f->i[0] > kMaxBins) return "GroundRemoval2: bin_num above the device limit of 4096";
      if ((long)f->i[0] * f->i[1] > kMaxFilterCells) return "GroundRemoval2: bin_num * segment_num above the device limit of 2^22";
      if (gr2_search_step(f->p[10], f->i[1]) > f->i[1]) return "GroundRemoval2: search_angle reaches past a whole turn";
      return nullptr;
    case SMHIP_FILTER_RANGE_IMAGE:
      if (f->i[0] <= 0 || f->i[1] <= 0) return "RangeImage: vertical_line_num and horizontal_line_num must be positive";
      if ((long)f->i[0] * f->i[1] > kMaxFilterCells) return "RangeImage: image larger than the device limit of 2^22 pixels";
      return nullptr;
    case SMHIP_FILTER_STATISTIC_REMOVAL:
      if (f->i[0] < 1 || f->i[0] > 64) return "StatisticRemoval: point_num_meank must be between 1 and the device limit of 64";
      if (!std::isfinite(f->p[0])) return "StatisticRemoval: std_mul must be finite";
      return nullptr;
  }
  smhip_filter_desc d;
  std::memset(&d, 0, sizeof(d));
  d.type = f->type; d.seed = f->seed; d.axis_index = f->i[0];
  for (int q = 0; q < 6; ++q) d.p[q] = f->p[q];
  return smhip_filter_config_valid(&d) ? nullptr : "ConfigsValid() is false";
}

static smhip_status filter_chain(smhip_handle h, const float* points, int stride_floats, int n, const smhip_filter_desc_ex* chain,
                                 int n_filters, int* n_out) {
  if (n > std::max(h->dev.ns_cap, h->dev.nt_cap)) { h->err = "cloud larger than the handle's capacity"; return SMHIP_ERR_CAPACITY; }
  HIPCHK(h, hipSetDevice(h->device));
  smhip_status s = filter_ensure(h);
  if (s) return s;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // stage rows as (x, y, z, intensity); the factors of stride-5 rows travel in the second half of the staging buffer
  float* fac = reinterpret_cast<float*>(h->stage + std::max(h->dev.ns_cap, h->dev.nt_cap));
  for (int i = 0; i < n; ++i) {
    const float* r = points + (size_t)stride_floats * i;
    h->stage[i] = make_float4(r[0], r[1], r[2], r[3]);
    if (stride_floats == 5) fac[i] = r[4];
  }
  HIPCHK(h, hipMemcpyAsync(h->prep_raw, h->stage, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  hipError_t e = filt_set_input(h->filt, h->stream, h->prep_raw, stride_floats == 5 ? fac : nullptr, n);
  if (e == hipSuccess) e = filt_run_chain(h->filt, h->stream, chain, n_filters, n_out);
  if (e != hipSuccess) { h->err = std::string("filter chain: ") + hipGetErrorString(e); return e == hipErrorInvalidValue ? SMHIP_ERR_INVALID_ARGUMENT : SMHIP_ERR_HIP; }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (n_out) *n_out = filt_count(h->filt);
  if (*filt_note(h->filt)) h->err = filt_note(h->filt);      // a warning: the call succeeded
  return SMHIP_OK;
}

smhip_status smhip_filter_chain_f32(smhip_handle h, const float* points, int stride_floats, int n, const smhip_filter_desc* chain,
                                    int n_filters, int* n_out) {
  if (!h || !points || n < 0 || n_filters < 0 || (n_filters > 0 && !chain) || (stride_floats != 4 && stride_floats != 5)) {
    if (h) h->err = "bad arguments (stride must be 4 = x y z intensity or 5 = InnerPointType)";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  for (int k = 0; k < n_filters; ++k)
    if (!smhip_filter_config_valid(&chain[k])) { h->err = "filter " + std::to_string(k) + ": ConfigsValid() is false"; return SMHIP_ERR_INVALID_ARGUMENT; }
  std::vector<smhip_filter_desc_ex> ex((size_t)n_filters);
  for (int k = 0; k < n_filters; ++k) ex[k] = widen(chain[k]);
  return filter_chain(h, points, stride_floats, n, ex.data(), n_filters, n_out);
}

void smhip_filter_default_ex(int type, smhip_filter_desc_ex* f) {
  if (!f) return;
  std::memset(f, 0, sizeof(*f));
  f->type = type;
  switch (type) {
    case SMHIP_FILTER_GROUND_REMOVAL:                                                         // filter_ground_removal.cc:28-38
      f->p[0] = 0.8f; f->p[1] = 0.15f; f->i[0] = 10; break;
    case SMHIP_FILTER_GROUND_REMOVAL2:                                                        // filter_ground_removal2.cc:72-110
      f->p[0] = 100.f; f->p[1] = 1.f; f->p[2] = -0.25f; f->p[3] = 1.0f; f->p[4] = 0.1f; f->p[5] = 0.2f; f->p[6] = 0.05f;
      f->p[7] = (float)std::tan(M_PI / 12.); f->p[8] = 0.1f; f->p[9] = 0.05f; f->p[10] = 10.f;
      f->i[0] = 200; f->i[1] = 180; f->i[2] = 4; break;
    case SMHIP_FILTER_RANGE_IMAGE:                                                            // filter_range_image.cc:28-52
      f->p[0] = 30.f; f->p[1] = -15.f; f->i[0] = 40; f->i[1] = 1800; break;
    case SMHIP_FILTER_STATISTIC_REMOVAL:                                                      // filter_statistic_removal.cc:31-37
      f->p[0] = 1.0f; f->i[0] = 30; break;
    default: {
      smhip_filter_desc d;
      smhip_filter_default(type, &d);
      *f = widen(d);
    }
  }
}

int smhip_filter_config_valid_ex(const smhip_filter_desc_ex* f) { return config_problem_ex(f) == nullptr ? 1 : 0; }

smhip_status smhip_filter_chain_ex_f32(smhip_handle h, const float* points, int stride_floats, int n, const smhip_filter_desc_ex* chain,
                                       int n_filters, int* n_out) {
  if (!h || !points || n < 0 || n_filters < 0 || (n_filters > 0 && !chain) || (stride_floats != 4 && stride_floats != 5)) {
    if (h) h->err = "bad arguments (stride must be 4 = x y z intensity or 5 = InnerPointType)";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  for (int k = 0; k < n_filters; ++k)
    if (const char* why = config_problem_ex(&chain[k])) { h->err = "filter " + std::to_string(k) + ": " + why; return SMHIP_ERR_INVALID_ARGUMENT; }
  return filter_chain(h, points, stride_floats, n, chain, n_filters, n_out);
}

smhip_status smhip_filter_get_output(smhip_handle h, float* points5, int32_t* source_index, int n) {
  if (!h || !h->filt) { if (h) h->err = "no filter chain has run"; return h ? SMHIP_ERR_NOT_READY : SMHIP_ERR_INVALID_ARGUMENT; }
  if (n != filt_count(h->filt)) { h->err = "n must equal the filtered size"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (n == 0) return SMHIP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<float4> p((size_t)n);
  std::vector<float> f((size_t)n);
  HIPCHK(h, hipMemcpyAsync(p.data(), filt_points(h->filt), sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(f.data(), filt_factors(h->filt), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  if (source_index) HIPCHK(h, hipMemcpyAsync(source_index, filt_source_index(h->filt), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (points5)
    for (int i = 0; i < n; ++i) {
      points5[5 * (size_t)i] = p[i].x; points5[5 * (size_t)i + 1] = p[i].y; points5[5 * (size_t)i + 2] = p[i].z;
      points5[5 * (size_t)i + 3] = p[i].w; points5[5 * (size_t)i + 4] = f[i];
    }
  return SMHIP_OK;
}

// parity hook: what the last StatisticRemoval of the last chain computed
smhip_status smhip_filter_statistic_last(smhip_handle h, float* distance, int n, double stats[4]) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  const int rows = h->filt ? filt_statistic_rows(h->filt) : -1;
  if (rows < 0) {
    h->err = rows == -2 ? "the last StatisticRemoval kept every row without computing distances (no more finite rows than point_num_meank)"
                        : "no StatisticRemoval ran in the last filter chain";
    return SMHIP_ERR_NOT_READY;
  }
  if (n != rows) { h->err = "n must equal the rows that filter saw (" + std::to_string(rows) + ")"; return SMHIP_ERR_INVALID_ARGUMENT; }
  HIPCHK(h, hipSetDevice(h->device));
  if (distance) HIPCHK(h, hipMemcpyAsync(distance, filt_statistic_distance(h->filt), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  if (stats) HIPCHK(h, hipMemcpyAsync(stats, filt_statistic_stats(h->filt), sizeof(double) * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SMHIP_OK;
}

// the filtered cloud becomes SetInputSource of `slot` without leaving the device
smhip_status smhip_filter_output_to_source(smhip_handle h, int slot) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!h->filt) { h->err = "no filter chain has run"; return SMHIP_ERR_NOT_READY; }
  const int n = filt_count(h->filt);
  if (n <= 0) { h->err = "the filtered cloud is empty"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (n > h->dev.ns_cap) { h->err = "filtered cloud larger than max_source_points"; return SMHIP_ERR_CAPACITY; }
  HIPCHK(h, hipSetDevice(h->device));
  const hipError_t e = prep_morton_sort(h->prep, h->stream, filt_points(h->filt), n, const_cast<float4*>(h->dev.src) + (size_t)slot * h->dev.ns_cap);
  if (e != hipSuccess) { h->err = std::string("prep_morton_sort: ") + hipGetErrorString(e); return SMHIP_ERR_HIP; }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->ns[slot] = n;
  touch_source(h, slot);
  return SMHIP_OK;
}

// MotionCompensation (map_builder.cc:232-257) of the filtered cloud -> SetInputSource of `slot`, on the device: the compensated
// rows go to the raw-scan staging array, from where prep_morton_sort orders them into the slot as it orders an uploaded scan
smhip_status smhip_filter_output_to_source_compensated(smhip_handle h, int slot, const double delta[16], float* points5_out) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!delta) { h->err = "null delta"; return SMHIP_ERR_INVALID_ARGUMENT; }
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(delta[k])) { h->err = "delta is not finite"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (!h->filt) { h->err = "no filter chain has run"; return SMHIP_ERR_NOT_READY; }
  const int n = filt_count(h->filt);
  if (n <= 0) { h->err = "the filtered cloud is empty"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (n > h->dev.ns_cap) { h->err = "filtered cloud larger than max_source_points"; return SMHIP_ERR_CAPACITY; }
  HIPCHK(h, hipSetDevice(h->device));
  hipError_t e = filt_motion_compensate(h->filt, h->stream, motion_comp_args(delta), h->prep_raw);
  if (e != hipSuccess) { h->err = std::string("filt_motion_compensate: ") + hipGetErrorString(e); return SMHIP_ERR_HIP; }
  // from here on the slot's source array is written: whatever source it held is gone, also when a factor is refused below
  h->ns[slot] = 0;
  touch_source(h, slot);
  e = prep_morton_sort(h->prep, h->stream, h->prep_raw, n, const_cast<float4*>(h->dev.src) + (size_t)slot * h->dev.ns_cap);
  if (e != hipSuccess) { h->err = std::string("prep_morton_sort: ") + hipGetErrorString(e); return SMHIP_ERR_HIP; }
  float* fac = reinterpret_cast<float*>(h->stage + std::max(h->dev.ns_cap, h->dev.nt_cap));
  if (points5_out) {
    HIPCHK(h, hipMemcpyAsync(h->stage, h->prep_raw, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(fac, filt_factors(h->filt), sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (filt_motion_bad_factor(h->filt)) {
    h->err = "a row's factor is outside [0, 1] or NaN (CHECK(factor >= 0. && factor <= 1.), common/math.h:202)";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  if (points5_out)
    for (int i = 0; i < n; ++i) {
      const float4 p = h->stage[i];
      float* o = points5_out + 5 * (size_t)i;
      o[0] = p.x; o[1] = p.y; o[2] = p.z; o[3] = p.w; o[4] = fac[i];
    }
  h->ns[slot] = n;
  touch_source(h, slot);
  return SMHIP_OK;
}

}  // extern "C"
