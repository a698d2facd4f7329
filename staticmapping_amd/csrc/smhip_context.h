// smhip_context.h -- what the host translation units of libsmhip.so share: the handle behind smhip_handle, the error and
// allocation helpers every entry point uses, and the handful of functions of the ICP unit (smhip_api.hip) that the NDT /
// NdtWithGicp unit (smhip_ndt_gicp.hip), the filter unit (smhip_filter_api.hip), the submap unit (smhip_submap.hip) and the descriptor unit (smhip_m2dp.hip) call.
// Internal: not installed, not part of the C ABI (include/smhip.h).  Everything else in those units is file-local.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/smhip.h"
#include "smhip_device.h"
#include "nabo_tree.h"
#include "prep_normals.h"
#include "cloud_filters.h"
#include "icp_plan.h"

using namespace smhip;          // (every includer is a host unit of the library written in terms of smhip's device types)

struct smhip_ndt_state;         // the NDT / NdtWithGicp unit's own (smhip_ndt_api.hip, smhip_gicp_api.hip): created on first use,
struct smhip_gicp_state;        // freed through smhip_internal_free_ndt / _gicp
struct smhip_m2dp_state;        // the descriptor unit's own (smhip_m2dp.hip): created on first use, freed through smhip_internal_free_m2dp
struct smhip_pose_graph_state;  // the pose-graph unit's own (smhip_pose_graph.hip): created on first use, freed through smhip_internal_free_pose_graph
struct smhip_guess_search_state;  // the guess-search unit's own (guess_search.hip): created on first use, freed through smhip_internal_free_guess_search

struct smhip_context {
  smhip_ndt_state* ndt = nullptr;
  smhip_gicp_state* gicp = nullptr;
  smhip_m2dp_state* m2dp = nullptr;
  smhip_pose_graph_state* pose_graph = nullptr;
  smhip_guess_search_state* guess_search = nullptr;
  PrepWorkspace* prep = nullptr;          // device CalculateNormals workspace (allocated on first use)
  PrepWorkspace* prep_batch = nullptr;    // the same sized for every slot at once (batched target preparation)
  FilterWorkspace* filt = nullptr;        // device pre-filters (allocated on first use)
  float4* prep_raw = nullptr;             // raw scan staging on the device
  float* submap_raw = nullptr;            // smhip_submap_build_f32: the frames' raw rows (5 floats per point of the filter workspace)
  void* submap_frames = nullptr;          // and its per-frame table (offset, n, pose), room for submap_frames_cap frames
  int submap_frames_cap = 0;
  float4* raw_batch = nullptr;            // the same for a whole batch of scans (smhip_set_sources_f32_batch; allocated on first use)
  hipStream_t copy_stream = nullptr;      // host-to-device copies of a batch of page-locked scans (overlap the handle's stream)
  hipEvent_t ev_copied = nullptr, ev_raw_free = nullptr;
  bool raw_in_use = false;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipStream_t side[plan::kMaxParts - 1] = {};      // the streams of a batch's parts beyond the first (icp_plan.h)
  hipEvent_t ev_fork = nullptr, ev_join[plan::kMaxParts - 1] = {};
  int n_side = 0;
  IcpDev dev{};
  KdDev kd{};                    // SMHIP_NN_NABO: tree arrays, allocated on first use
  bool kd_allocated = false;
  smhip_icp_options opts{};
  std::vector<int> ns, nt, has_normals;
  // Target-side structures are kept across calls while a slot's target is unchanged (single-pair calls only: the front end
  // aligns scan after scan against one key frame, map_builder.cc:379-392).  tgt_gen[slot] changes whenever the slot's target
  // does; grid_gen / grid_cell / grid_sorted describe the search structure currently resident in the slot.
  std::vector<unsigned long long> tgt_gen, grid_gen;
  std::vector<unsigned long long> src_gen, src3_gen;   // same idea for the packed 12-byte copy of a slot's source (pack_source)
  std::vector<float> grid_cell_built;
  std::vector<int> grid_sorted, grid_rows, grid_mode;   // grid_rows: row-occupancy bitmap built too; grid_mode: nn_mode of the structure
  unsigned long long gen_counter = 0;
  int nabo_listed_blocks = kNaboListedBlocks;   // workgroups per pair of the list walk (SMHIP_NABO_LISTED_BLOCKS overrides, tuning only)
  int target_cache = 1;             // smhip_set_target_cache
  int inner_comp = 0;               // smhip_icp_set_inner_compensation: Aligns de-skew the source inside every iteration (dev.comp3 allocated)
  unsigned long long cache_hits = 0;
  PairInput* in_pinned = nullptr;
  PairState* state_pinned = nullptr;
  int hist_mode = 0;             // nn_mode of the batch whose searched-query history is waiting in hist_pinned
  int nabo_fused_from = 6;       // reference-search mode: the first iteration of a batch that runs the fused certificate pass (plan::fused_now)
  float split_share = 0.2f;      // auto split: the first iteration whose median searched share falls below this runs certify + listed search
  int sums_blocks = kSumsBlocks;  // workgroups of iteration_sums (SMHIP_SUMS_BLOCKS)
  int sums_long_for = 3;         // fused iterations of a batch whose missed pairs iteration_sums cuts into long blocks (SMHIP_SUMS_LONG_FOR)
  int use_shadow = 1;            // fused certificate pass reads the 4-byte shadow of (bound, match) where every target is small enough (SMHIP_SHADOW)
  int one_blocks = 0;            // workgroups of the single-pair persistent kernel the device holds at once (0: not available)
  int one_used = 0;              // the last single-pair enqueue went through it
  int one_blocks_allowed = 1;    // 0: fine-grained memory could not be had at smhip_create
  long long one_launches = 0;    // enqueues that went through it (smhip_icp_single_launch_counts)
  int one_fallbacks = 0;         // Aligns done again as separate launches because the launch stopped itself (see fetch_range)
  int one_enabled = 1;           // SMHIP_ONE_PAIR=0: single pairs through the separate launches (measurement aid)
  int one_groups_want = 0;       // SMHIP_ONE_GROUPS: groups of its barrier (tuning)
  int one_blocks_want = 0;       // SMHIP_ONE_BLOCKS: its grid (tuning; 0 = as many as a round each needs, at most what is resident)
  int one_pairs_max = kOnePairs; // SMHIP_ONE_PAIRS: pairs one launch of it may hold (1 = single pairs only)
  int one_idle = 0;              // SMHIP_ONE_IDLE: with SMHIP_ONE_BLOCKS, keep a grid of mostly idle workgroups on small clouds (tests)
  int one_no_retry = 0;          // SMHIP_ONE_NO_RETRY: a launch that stopped itself is reported, not done again (fetch_range)
  int grid_sort_build = 1;       // 0 (SMHIP_GRID_BUILD=0): every grid build through the mark / rank / count / place kernels (measurement aid)
  bool build_sorted = false;     // what the last enqueue_resets chose for the grid build that follows it (plan::sorted_grid_build)
  int wave_search = 0;           // batches: the every-query-searches iterations through nn_ball_lds (0, default: 5-25 % faster on the bench scans)
                                 // or nn_ball_wave (1; SMHIP_WAVE_SEARCH=1) -- same results
  float4* stage = nullptr;       // pinned staging for uploads, 2 * max(ns_cap, nt_cap)
  uint32_t* done_pinned = nullptr;
  // split_after = 0: where the batched iterations switch from the fused search to certify + listed search follows the
  // previous batch (the share of queries that needed a search per iteration, search_hist): a front end's guesses are
  // alike from call to call.  Results do not depend on it, only the time.
  uint32_t* hist_pinned = nullptr;
  int hist_first = 0;
  int hist_pairs = 0;                  // pairs whose rows the last enqueue copied to hist_pinned (0 = none)
  std::vector<int> hist_ns;            // their sources' sizes at that enqueue (the slots may hold other clouds by the time the rows are read)
  int hist_iters = 0;                  // iterations that enqueue ran
  int auto_split = 2;
  int32_t* ids_pinned = nullptr;
  float* d2_pinned = nullptr;
  int32_t* ids_dev = nullptr;    // scratch for exported matches
  float* d2_dev = nullptr;
  smhip_icp_information* info_dev = nullptr;   // [slots] results of the information unit (smhip_icp_information.hip), allocated on first use
  std::vector<void*> allocs;
  std::string err;
  int last_npairs = 0;
  // profiling
  int profile = 0;               // 0 off, 1 every launch, 2 the dominant NN kernel only
  struct Ev { hipEvent_t a, b; int cat; int np; };
  std::vector<Ev> ev_pool;
  size_t ev_used = 0;
  smhip_icp_profile prof{};
};

#define HIPCHK(h, expr)                                                                   \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) {                                                               \
      (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                       \
      return SMHIP_ERR_HIP;                                                               \
    }                                                                                     \
  } while (0)

// (hidden: calls between the units bind inside the library and nothing here joins its exported symbols)
namespace smhip_host __attribute__((visibility("hidden"))) {

template <typename T>
smhip_status dev_alloc(smhip_context* h, T** p, size_t count) {
  void* v = nullptr;
  HIPCHK(h, hipMalloc(&v, count * sizeof(T)));
  h->allocs.push_back(v);
  *p = reinterpret_cast<T*>(v);
  return SMHIP_OK;
}

inline void touch_target(smhip_context* h, int slot) { h->tgt_gen[slot] = ++h->gen_counter; }
inline void touch_source(smhip_context* h, int slot) { h->src_gen[slot] = ++h->gen_counter; }
inline void touch_grid(smhip_context* h, int first, int np) {        // the slots' search structures are (re)built / overwritten
  for (int p = first; p < first + np; ++p) { h->grid_gen[p] = 0; h->grid_cell_built[p] = 0.f; h->grid_sorted[p] = 0; h->grid_rows[p] = 0; h->grid_mode[p] = -1; }
}

// One half of a batch: a by-value copy of the device view restricted to pairs [pair_base, pair_base + np)
// and the stream its launches go to.
struct Half {
  IcpDev d;
  hipStream_t stream;
  int np;
  plan::Part part;         // how its launches size themselves (enqueue_range)
  int first_fused = -1;    // the first iteration of this Align that ran the fused path
};

// Defined in smhip_filter_api.hip: the filter workspace (and prep_ensure's), allocated on first use.
smhip_status filter_ensure(smhip_context* h);
// Defined in smhip_api.hip (the ICP unit), where each is described.
smhip_status check_slot(smhip_context* h, int slot);
smhip_status prep_ensure(smhip_context* h);
smhip_status prep_run(smhip_context* h, const float4* raw_dev, int n, int slot, int* n_out);
smhip_status enqueue_resets(smhip_context* h, int np, int first = 0, int nt_max = -1);
smhip_status enqueue_grid_build(smhip_context* h, const Half& f, int nt_max);
bool grid_cached(smhip_context* h, int slot);
smhip_status enqueue_prepare_kept(smhip_context* h, int first, int K);
Half whole_batch(smhip_context* h, int np, int first);
smhip_status enqueue_find_closests_half(smhip_context* h, const Half& f, int ns_max);
smhip_status fill_inputs(smhip_context* h, int np, const double* guesses, int* ns_max, int* nt_max, int first = 0);
smhip_status trimmed_pass_range(smhip_context* h, int first, int npairs, const double* Ts, float dist_outlier_ratio, smhip_icp_stats* stats);

}  // namespace smhip_host
