// smhip_api.hip -- host side of the C ABI declared in include/smhip.h.
//
// One smhip_context = one matcher instance in the sense of
// static_map::registrator::Interface (/root/reference/registrators/interface.h:67-116):
// it owns a stream, a device arena sized at creation (no hipMalloc inside Align) and
// `slots` independent scan pairs.  The IcpFast loop (icp_fast.cc:455-529) stays resident on
// the device; the host only enqueues launches and, when early exit is on, polls one word
// every `check_every` iterations.
//
// This file is the ICP translation unit of libsmhip.so: it defines the kernels of icp_kernels.hip and of the three fragments
// that reuse their bodies (grid_sort_build.hip, icp_one.hip, nabo_kernels.hip), in that order, and the entry points of IcpFast and of the clouds
// every matcher shares.  The other host units (smhip_ndt_gicp.hip, smhip_filter_api.hip) reach the handle and the functions of
// namespace smhip_host below through smhip_context.h.
#include "icp_kernels.hip"
#include "grid_sort_build.hip"
#include "icp_one.hip"
#include "nabo_kernels.hip"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "smhip_context.h"

using namespace smhip_host;
using plan::ceil_div;

static_assert(plan::kRingCoopLanes == kCoopLanes && plan::kNaboBucket == kKdBucket && plan::kNaboShallowLevels <= kKdStack,
              "icp_plan.h restates kernel constants");
static_assert(plan::kSortBuildMaxTarget == kGsMaxPoints, "icp_plan.h restates grid_sort_build's capacity");

namespace {

thread_local std::string g_create_error;

// profiling brackets around launches of one category (plan::Category)
struct Bracket {
  smhip_context* h;
  smhip_context::Ev* ev = nullptr;
  hipStream_t st;
  Bracket(smhip_context* h_, int cat, hipStream_t st_, int np = 0) : h(h_), st(st_) {
    // 1: every launch.  2 / 3 / 4: ONE kernel class only -- the NN kernels proper (fused search / full walk and the certificate
    // pass), accumulate, or the listed search -- which costs a timed region one event pair per iteration and part (every
    // bracket is a barrier between two launches: all classes at once took 6 % off the batch rate)
    if (!h->profile) return;
    if (h->profile == 2 && cat != 4 && cat != 5) return;
    if (h->profile == 3 && cat != 2) return;
    if (h->profile == 4 && cat != 6) return;
    if (h->ev_used == h->ev_pool.size()) {
      smhip_context::Ev e{};
      if (hipEventCreate(&e.a) != hipSuccess || hipEventCreate(&e.b) != hipSuccess) return;
      h->ev_pool.push_back(e);
    }
    ev = &h->ev_pool[h->ev_used++];
    ev->cat = cat;
    ev->np = np;
    (void)hipEventRecord(ev->a, st);
  }
  ~Bracket() {
    if (ev) (void)hipEventRecord(ev->b, st);
  }
};

void collect_profile(smhip_context* h) {
  if (!h->profile) return;
  for (size_t k = 0; k < h->ev_used; ++k) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, h->ev_pool[k].a, h->ev_pool[k].b) != hipSuccess) continue;
    switch (h->ev_pool[k].cat) {
      case 0: h->prof.ms_prepare += ms; break;
      case 1: h->prof.ms_find_closests += ms; h->prof.launches_find_closests++; h->prof.ms_nn_refine += ms; h->prof.launches_nn_refine++; break;
      case 6: h->prof.ms_find_closests += ms; h->prof.launches_find_closests++;
              h->prof.ms_nn_listed += ms; h->prof.launches_nn_listed++; h->prof.pairs_nn_listed += h->ev_pool[k].np; break;
      case 4: h->prof.ms_find_closests += ms; h->prof.launches_find_closests++;
              h->prof.ms_nn_main += ms; h->prof.launches_nn_main++; h->prof.pairs_nn_main += h->ev_pool[k].np; break;
      case 5: h->prof.ms_find_closests += ms; h->prof.launches_find_closests++;
              h->prof.ms_nn_certify += ms; h->prof.launches_nn_certify++; h->prof.pairs_nn_certify += h->ev_pool[k].np; break;
      case 2: h->prof.ms_error_elements += ms; h->prof.launches_error_elements++; h->prof.pairs_error_elements += h->ev_pool[k].np; break;
      case 3: h->prof.ms_solve += ms; h->prof.launches_solve++; break;
    }
  }
  h->ev_used = 0;
}

}  // namespace

// What the other host units call is declared in smhip_context.h; the helpers marked static are this file's own.
namespace smhip_host {

smhip_status check_slot(smhip_context* h, int slot) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  if (slot < 0 || slot >= h->dev.slots) { h->err = "slot out of range"; return SMHIP_ERR_INVALID_ARGUMENT; }
  return SMHIP_OK;
}

// the ICP iteration kernels stream the 12-byte copy of the sources: repacked here (main stream, the PairInput rows already
// on their way) for launches that cover a slot whose source changed since it was last packed
static smhip_status ensure_packed(smhip_context* h, int first, int np) {
  bool stale = false;
  for (int p = first; p < first + np; ++p) stale = stale || h->src3_gen[p] != h->src_gen[p];
  if (!stale) return SMHIP_OK;
  hipLaunchKernelGGL(pack_source, dim3(std::min(8192, 128 * np)), dim3(256), 0, h->stream, h->dev, first, np);
  HIPCHK(h, hipGetLastError());
  for (int p = first; p < first + np; ++p) h->src3_gen[p] = h->src_gen[p];
  return SMHIP_OK;
}

// per-call resets for pairs [first, first + np) (main stream, before the halves fork).  nt_max >= 0: the largest target of the grid
// build that follows, which decides here, once for all its parts, which form that build takes (plan::sorted_grid_build): the
// sorted form needs neither `bits` nor `ccount` zeroed -- 1 MiB + nt_cap words per pair -- and gets the light reset.
smhip_status enqueue_resets(smhip_context* h, int np, int first, int nt_max) {
  IcpDev& d = h->dev;
  touch_grid(h, first, np);               // the build that follows overwrites whatever structure was resident
  HIPCHK(h, hipMemcpyAsync(const_cast<PairInput*>(d.in) + first, h->in_pinned + first, sizeof(PairInput) * np, hipMemcpyHostToDevice, h->stream));
  h->build_sorted = nt_max >= 0 && plan::sorted_grid_build(h->grid_sort_build, h->opts.nn_mode, d.sort_cells, d.use_ball ? 0 : 1, np, nt_max);
  if (h->build_sorted) hipLaunchKernelGGL(reset_scratch_light, dim3(std::min(1024, 8 * np)), dim3(256), 0, h->stream, d, first, np);
  else hipLaunchKernelGGL(reset_scratch, dim3(std::min(4096, 256 * np)), dim3(256), 0, h->stream, d, first, np);
  return ensure_packed(h, first, np);
}

// target centring + search-structure build for one half
static smhip_status kd_ensure(smhip_context* h) {
  if (h->kd_allocated) return SMHIP_OK;
  const size_t B = h->dev.slots, NT = h->dev.nt_cap;
  h->kd.node_cap = (int32_t)(NT / 2 + 8);       // a split node has >= 9 points and gives each child >= 4: <= nt / 4 leaves, 2 leaves - 1 nodes
  h->kd.seg_cap = (int32_t)(NT / 4 + 8);
  smhip_status s = SMHIP_OK;
  auto A = [&](smhip_status r) { if (s == SMHIP_OK) s = r; };
  A(dev_alloc(h, &h->kd.nodes, B * (size_t)h->kd.node_cap));
  A(dev_alloc(h, &h->kd.segs, B * 2 * (size_t)h->kd.seg_cap));
  A(dev_alloc(h, &h->kd.alt, B * NT));
  A(dev_alloc(h, &h->kd.cnt, B * 2 * (size_t)h->kd.seg_cap));
  h->kd.leaf_cap = (int32_t)(NT / 4 + 2);       // block index = bucket start >> 2
  A(dev_alloc(h, &h->kd.leaf, B * (size_t)h->kd.leaf_cap * 24));
  A(dev_alloc(h, &h->dev.nabo_work, B * (size_t)h->dev.ns_cap));
  if (s == SMHIP_OK) h->kd_allocated = true;
  return s;
}

smhip_status enqueue_grid_build(smhip_context* h, const Half& f, int nt_max) {
  const IcpDev& d = f.d;
  const int np = f.np;
  Bracket br(h, plan::kCatPrepare, f.stream);
  const dim3 gpts(ceil_div(nt_max, 256), np);
  hipLaunchKernelGGL(tgt_reduce, dim3(kTgtReduceBlocks, np), dim3(256), 0, f.stream, d);
  if (h->build_sorted) {
    // the form enqueue_resets chose for this call (and left `bits` / `ccount` unzeroed for): setup, sort and fill as one launch
    if (h->opts.nn_mode == SMHIP_NN_NABO || !d.sort_cells || d.have_rowbits || nt_max > kGsMaxPoints) {
      h->err = "grid build: the settings changed between the reset and the build"; return SMHIP_ERR_NOT_READY;
    }
    hipLaunchKernelGGL(grid_sort_build, dim3(np), dim3(kGsThreads), 0, f.stream, d);
    HIPCHK(h, hipGetLastError());
    for (int p = d.pair_base; p < d.pair_base + np; ++p) {
      h->grid_gen[p] = h->tgt_gen[p]; h->grid_cell_built[p] = d.grid_cell; h->grid_sorted[p] = d.sort_cells; h->grid_rows[p] = d.have_rowbits;
      h->grid_mode[p] = SMHIP_NN_GRID;
    }
    return SMHIP_OK;
  }
  hipLaunchKernelGGL(grid_setup, dim3(ceil_div(np, 64)), dim3(64), 0, f.stream, d, np);
  if (h->opts.nn_mode == SMHIP_NN_NABO) {
    // the reference's own structure: libnabo's kd-tree over the centred target, rebuilt per Align (icp_fast.cc:464-467)
    if (!h->kd_allocated) { h->err = "nn_mode NABO: tree arrays missing (smhip_icp_set_options allocates them)"; return SMHIP_ERR_NOT_READY; }
    // the search keeps one pending sibling per tree level in kKdStack LDS slots per query; a median split halves (rounding
    // up) until a bucket holds <= 8 points, so 8 << kKdStack points is the deepest tree the stack can follow
    if (nt_max > (kKdBucket << kKdStack)) { h->err = "nn_mode NABO: target larger than 8 << 18 points (the search stack holds 18 tree levels)"; return SMHIP_ERR_CAPACITY; }
    hipLaunchKernelGGL(kd_build, dim3(np), dim3(kKdThreads), 0, f.stream, d, h->kd);
    HIPCHK(h, hipGetLastError());
    for (int p = d.pair_base; p < d.pair_base + np; ++p) {
      h->grid_gen[p] = h->tgt_gen[p]; h->grid_cell_built[p] = d.grid_cell; h->grid_sorted[p] = 1; h->grid_rows[p] = 0; h->grid_mode[p] = SMHIP_NN_NABO;
    }
    return SMHIP_OK;
  }
  hipLaunchKernelGGL(grid_mark, gpts, dim3(256), 0, f.stream, d);
  // the ring searches (NDT fitness, GICP neighbourhoods / correspondences) skip empty grid rows through a bitmap; the ball
  // search of IcpFast visits a handful of rows per query and does not need it
  if (d.have_rowbits) hipLaunchKernelGGL(grid_rowbits, dim3(ceil_div(kMaxRowWords, 256), np), dim3(256), 0, f.stream, d);
  hipLaunchKernelGGL(grid_rank, dim3(std::max(1, std::min(16, 64 / np)), np), dim3(1024), 0, f.stream, d);   // segments per pair when pairs are few
  hipLaunchKernelGGL(grid_count, gpts, dim3(256), 0, f.stream, d);
  hipLaunchKernelGGL(grid_cscan, dim3(np), dim3(1024), 0, f.stream, d);
  if (d.sort_cells) {
    hipLaunchKernelGGL(grid_scatter_idx, gpts, dim3(256), 0, f.stream, d);
    hipLaunchKernelGGL(grid_place, gpts, dim3(256), 0, f.stream, d);
  } else {
    hipLaunchKernelGGL(grid_scatter, gpts, dim3(256), 0, f.stream, d);
  }
  HIPCHK(h, hipGetLastError());
  for (int p = d.pair_base; p < d.pair_base + np; ++p) {
    h->grid_gen[p] = h->tgt_gen[p]; h->grid_cell_built[p] = d.grid_cell; h->grid_sorted[p] = d.sort_cells; h->grid_rows[p] = d.have_rowbits;
    h->grid_mode[p] = SMHIP_NN_GRID;
  }
  return SMHIP_OK;
}

// is the search structure resident in `slot` the one a build with the current settings would produce?
bool grid_cached(smhip_context* h, int slot) {
  const int want_mode = h->opts.nn_mode == SMHIP_NN_NABO ? SMHIP_NN_NABO : SMHIP_NN_GRID;   // which structure: kd-tree or grid
  if (h->grid_mode[slot] != want_mode) return false;
  if (want_mode == SMHIP_NN_NABO) return h->target_cache && h->grid_gen[slot] != 0 && h->grid_gen[slot] == h->tgt_gen[slot];
  return h->target_cache && h->grid_gen[slot] != 0 && h->grid_gen[slot] == h->tgt_gen[slot] &&
         h->grid_cell_built[slot] == h->dev.grid_cell && h->grid_sorted[slot] >= h->dev.sort_cells &&
         h->grid_rows[slot] >= (h->dev.use_ball ? 0 : 1);
}

// "target kept" prepare of slots [first, first + K), whose search structures are all current: pair inputs, pose and the light scratch reset
smhip_status enqueue_prepare_kept(smhip_context* h, int first, int K) {
  const IcpDev d = whole_batch(h, K, first).d;
  HIPCHK(h, hipMemcpyAsync(const_cast<PairInput*>(d.in) + first, h->in_pinned + first, sizeof(PairInput) * K, hipMemcpyHostToDevice, h->stream));
  { smhip_status ps = ensure_packed(h, first, K); if (ps) return ps; }
  hipLaunchKernelGGL(reset_scratch_light, dim3(std::min(1024, 8 * K)), dim3(256), 0, h->stream, d, first, K);
  hipLaunchKernelGGL(pose_setup, dim3(ceil_div(K, 64)), dim3(64), 0, h->stream, d, K);
  HIPCHK(h, hipGetLastError());
  h->cache_hits++;
  return SMHIP_OK;
}

// single-pair form of enqueue_resets + enqueue_grid_build that skips the build when the slot's target is unchanged
static smhip_status enqueue_prepare_one(smhip_context* h, int slot, int nt_max) {
  if (grid_cached(h, slot)) return enqueue_prepare_kept(h, slot, 1);
  smhip_status s = enqueue_resets(h, 1, slot, nt_max);
  if (s) return s;
  return enqueue_grid_build(h, whole_batch(h, 1, slot), nt_max);
}

Half whole_batch(smhip_context* h, int np, int first) {
  Half f;
  f.d = h->dev; f.d.npairs = np; f.d.pair_base = first;
  f.d.have_rowbits = h->dev.use_ball ? 0 : 1;     // ring-search contexts build and use the row-occupancy bitmap
  f.stream = h->stream; f.np = np;
  return f;
}

// single-stream convenience used by find_closests / the NDT fitness pass
static smhip_status enqueue_prepare(smhip_context* h, int np, int nt_max) {
  if (np == 1) return enqueue_prepare_one(h, 0, nt_max);
  smhip_status s = enqueue_resets(h, np, 0, nt_max);
  if (s) return s;
  return enqueue_grid_build(h, whole_batch(h, np, 0), nt_max);
}

static inline int nt_max_of(const smhip_context* h, int first, int np) {
  int m = 0;
  for (int p = first; p < first + np; ++p) m = std::max(m, h->nt[p]);
  return m;
}

// the settings the plan reads, as they stand now (callers that patch h->dev or h->opts around a search patch the plan's inputs)
static plan::Inputs plan_inputs(const smhip_context* h) {
  plan::Inputs in;
  in.nn_mode = h->opts.nn_mode;
  in.use_ball = h->dev.use_ball; in.lds_table = h->dev.lds_table; in.certify = h->dev.certify; in.exact_all = h->dev.exact_all;
  in.split_after = h->dev.split_after; in.split_after_option = h->opts.split_after;
  in.no_fused_sums = h->opts.no_fused_sums; in.no_single_kernel = h->opts.no_single_kernel;
  in.no_overlap = h->opts.no_overlap; in.overlap_streams = h->opts.overlap_streams;
  in.nabo_fused_from = h->nabo_fused_from; in.sums_long_for = h->sums_long_for; in.use_shadow = h->use_shadow; in.wave_search = h->wave_search;
  in.sums_blocks = h->sums_blocks; in.nabo_listed_blocks = h->nabo_listed_blocks;
  in.one_enabled = h->one_enabled; in.one_blocks_want = h->one_blocks_want; in.one_groups_want = h->one_groups_want;
  in.one_idle = h->one_idle; in.one_pairs_max = h->one_pairs_max; in.one_blocks = h->one_blocks;
  in.profiling = h->profile != 0;
  in.part_stride = h->dev.part_stride; in.seg_stride = h->dev.seg_stride;
  in.side_streams = h->n_side;
  in.compensation = h->inner_comp;
  return in;
}

// (1 + epsilon)^2 as the searches of nn_mode NABO multiply by it
static float kd_max_error2(const smhip_context* h) {
  const float e = h->opts.nn_epsilon >= 0.f ? h->opts.nn_epsilon : 3.16f;
  return (1.0f + e) * (1.0f + e);
}

// launches what a plan names, in its order, on the part's stream
static smhip_status enqueue_launches(smhip_context* h, const Half& f, const plan::Iteration& it) {
  using K = plan::Kernel;
  const IcpDev& d = f.d;
  hipStream_t st = f.stream;
  KdDev kd = h->kd;
  kd.max_error2 = kd_max_error2(h);
  constexpr int kShallow = plan::kNaboShallowLevels;
  const dim3 nn(kNnThreads), acc(kAccThreads), t256(256);
  std::optional<Bracket> br;
  for (int i = 0; i < it.n; ++i) {
    const plan::Launch& l = it.launch[i];
    if (!l.same_bracket) { br.reset(); br.emplace(h, l.cat, st, f.np); }
    const dim3 g(l.gx, l.gy);
    switch (l.kernel) {
      case K::NaboCertifyOne:     hipLaunchKernelGGL((nn_certify<1, true>), g, nn, 0, st, d, l.nb); break;
      case K::NaboCertifyAcc:     hipLaunchKernelGGL((nn_certify_acc<kCertifyItems, true>), g, nn, 0, st, d, l.nb); break;
      case K::NaboCertify:        hipLaunchKernelGGL((nn_certify<kCertifyItems, true>), g, nn, 0, st, d, l.nb); break;
      case K::NaboListedShallow:  hipLaunchKernelGGL((nn_nabo<1, true, kShallow>), g, nn, 0, st, d, kd, l.nb); break;
      case K::NaboListedDeep:     hipLaunchKernelGGL((nn_nabo<1, true, kKdStack>), g, nn, 0, st, d, kd, l.nb); break;
      case K::NaboValidate:       hipLaunchKernelGGL(nabo_validate, g, acc, 0, st, d); break;
      case K::AccumulateListed:   hipLaunchKernelGGL(accumulate_listed, g, acc, 0, st, d); break;
      case K::NaboOneShallow:     hipLaunchKernelGGL((nn_nabo<1, false, kShallow>), g, nn, 0, st, d, kd, l.nb); break;
      case K::NaboOneDeep:        hipLaunchKernelGGL((nn_nabo<1, false, kKdStack>), g, nn, 0, st, d, kd, l.nb); break;
      case K::NaboFourShallow:    hipLaunchKernelGGL((nn_nabo<4, false, kShallow>), g, nn, 0, st, d, kd, l.nb); break;
      case K::NaboFourDeep:       hipLaunchKernelGGL((nn_nabo<4, false, kKdStack>), g, nn, 0, st, d, kd, l.nb); break;
      case K::BallLdsOne:         hipLaunchKernelGGL(nn_ball_lds<1>, g, nn, 0, st, d, l.nb); break;
      case K::BallWaveFirst:      hipLaunchKernelGGL((nn_ball_wave<kBallItems, true>), g, nn, 0, st, d, l.nb); break;
      case K::BallWave:           hipLaunchKernelGGL((nn_ball_wave<kBallItems, false>), g, nn, 0, st, d, l.nb); break;
      case K::BallLdsFirst:       hipLaunchKernelGGL((nn_ball_lds<kBallItems, true>), g, nn, 0, st, d, l.nb); break;
      case K::BallLds:            hipLaunchKernelGGL(nn_ball_lds<kBallItems>, g, nn, 0, st, d, l.nb); break;
      case K::CertifyAccShadow:   hipLaunchKernelGGL((nn_certify_acc<kCertifyItems, false, true>), g, nn, 0, st, d, l.nb); break;
      case K::CertifyAcc:         hipLaunchKernelGGL(nn_certify_acc<kCertifyItems>, g, nn, 0, st, d, l.nb); break;
      case K::CertifyOne:         hipLaunchKernelGGL(nn_certify<1>, g, nn, 0, st, d, l.nb); break;
      case K::Certify:            hipLaunchKernelGGL(nn_certify<kCertifyItems>, g, nn, 0, st, d, l.nb); break;
      case K::ListedPlan:         hipLaunchKernelGGL(listed_plan, g, t256, 0, st, d); break;
      case K::BallListedItems:    hipLaunchKernelGGL(nn_ball_listed_items, g, nn, 0, st, d); break;
      case K::BallListed:         hipLaunchKernelGGL(nn_ball_listed, g, nn, 0, st, d, l.nb); break;
      case K::Ball:               hipLaunchKernelGGL(nn_ball, g, nn, 0, st, d, l.nb); break;
      case K::RefineOne:          hipLaunchKernelGGL(nn_refine_one, g, nn, 0, st, d); break;
      case K::Validate:           hipLaunchKernelGGL(nn_validate, g, t256, 0, st, d); break;
      case K::RingRefine:         hipLaunchKernelGGL(nn_ring<true>, g, nn, 0, st, d); break;
      case K::RingCoop:           hipLaunchKernelGGL(nn_ring_coop, g, nn, 0, st, d); break;
      case K::RingWide:           hipLaunchKernelGGL(nn_ring_wide, g, nn, 0, st, d); break;
      case K::Ring:               hipLaunchKernelGGL(nn_ring<false>, g, nn, 0, st, d); break;
      case K::Fallback:           hipLaunchKernelGGL(nn_fallback, g, nn, 0, st, d); break;
      case K::Brute:              hipLaunchKernelGGL(nn_brute, g, nn, 0, st, d); break;
      case K::IterationSumsBatch: hipLaunchKernelGGL(iteration_sums<kAccItemsBatch>, g, acc, 0, st, d); break;
      case K::IterationSumsSmall: hipLaunchKernelGGL(iteration_sums<kAccItemsSmall>, g, acc, 0, st, d); break;
      case K::AccumulateBatch:    hipLaunchKernelGGL(accumulate<kAccItemsBatch>, g, acc, 0, st, d, l.nb); break;
      case K::AccumulateSmall:    hipLaunchKernelGGL(accumulate<kAccItemsSmall>, g, acc, 0, st, d, l.nb); break;
      case K::Finalize:           hipLaunchKernelGGL(finalize, g, t256, 0, st, d); break;
      case K::CompApply:          hipLaunchKernelGGL(comp_apply, g, t256, 0, st, d); break;
      case K::AccumulateCompBatch: hipLaunchKernelGGL(accumulate_comp<kAccItemsBatch>, g, acc, 0, st, d, l.nb); break;
      case K::AccumulateCompSmall: hipLaunchKernelGGL(accumulate_comp<kAccItemsSmall>, g, acc, 0, st, d, l.nb); break;
      case K::FinalizeComp:       hipLaunchKernelGGL(finalize_comp, g, t256, 0, st, d); break;
    }
  }
  return SMHIP_OK;
}

// FindClosests outside an Align (find_closests, the GICP correspondences): iteration 0 of one launch over pairs [f.d.pair_base, + f.np)
smhip_status enqueue_find_closests_half(smhip_context* h, const Half& f, int ns_max) {
  return enqueue_launches(h, f, plan::plan_search_only(plan_inputs(h), plan::whole_part(f.np, nt_max_of(h, f.d.pair_base, f.np)), ns_max));
}

static smhip_status enqueue_find_closests(smhip_context* h, int np, int ns_max) {
  return enqueue_find_closests_half(h, whole_batch(h, np, 0), ns_max);
}

smhip_status fill_inputs(smhip_context* h, int np, const double* guesses, int* ns_max, int* nt_max, int first) {
  *ns_max = 0; *nt_max = 0;
  for (int p = first; p < first + np; ++p) {
    if (h->ns[p] <= 0 || h->nt[p] <= 0) { h->err = "Align before SetInputSource/SetInputTarget"; return SMHIP_ERR_NOT_READY; }
    if (!h->has_normals[p]) { h->err = "IcpFast target has no normals (icp_fast.cc:430)"; return SMHIP_ERR_NO_NORMALS; }
    PairInput& in = h->in_pinned[p];
    const double* g = guesses + 16 * (p - first);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) in.guess[4 * r + c] = g[4 * c + r];   // column-major in
    in.ns = h->ns[p]; in.nt = h->nt[p]; in.has_normals = 1; in.pad = 0;
    *ns_max = std::max(*ns_max, h->ns[p]);
    *nt_max = std::max(*nt_max, h->nt[p]);
  }
  return SMHIP_OK;
}

// the single-cloud CalculateNormals / Morton-order workspace and the raw staging array: allocated on first use
smhip_status prep_ensure(smhip_context* h) {
  if (h->prep) return SMHIP_OK;
  const int cap = std::max(h->dev.ns_cap, h->dev.nt_cap);
  h->prep = prep_create(cap);
  if (!h->prep) { h->err = "device CalculateNormals workspace allocation failed"; return SMHIP_ERR_HIP; }
  return dev_alloc(h, &h->prep_raw, (size_t)cap);
}

static void sync_options(smhip_context* h) {
  h->dev.max_iteration = std::max(1, h->opts.max_iteration);
  h->dev.early_exit = h->opts.early_exit;
  h->dev.max_ring = std::max(1, h->opts.grid_max_ring);
  h->dev.rho = h->opts.dist_outlier_ratio;
  h->dev.grid_cell = h->opts.grid_cell > 0 ? h->opts.grid_cell : 0.5f;
  h->dev.use_ball = h->opts.use_ball;
  h->dev.sort_cells = 1;
  h->dev.certify = h->opts.no_certify ? 0 : 1;
  h->dev.split_after = h->opts.split_after > 0 ? h->opts.split_after : (h->opts.split_after < 0 ? 1 << 30 : 2);
  h->dev.lds_table = h->opts.no_lds_table ? 0 : 1;
  h->dev.cap_factor = h->opts.ball_cap_factor > 1.0f ? h->opts.ball_cap_factor : 1.5f;
  h->dev.exact_all = h->opts.exact_matches;
  h->dev.ball_radius = h->opts.ball_radius > 0 ? h->opts.ball_radius : 0.3f;
  // (the ball search walks a query's rows through a 32-bit mask: at most 14 cells of radius, 3.5 m with the default cell -- a larger
  // radius only moves the point from which the ring search takes over, never the result)
  h->dev.ball_radius = std::min(h->dev.ball_radius, 14.0f * h->dev.grid_cell);
  { const char* e = std::getenv("SMHIP_DEBUG_FLAGS"); h->dev.debug_flags = e ? std::atoi(e) : 0; }
  h->dev.fused = 0; h->dev.fused_nabo = 0;
  h->dev.band_pad = 0.1f; h->dev.band_gain = 1.5f;              // tuning only: results do not depend on the band, only how often it holds
  { const char* e = std::getenv("SMHIP_BAND_PAD"); if (e && std::atof(e) >= 0.0) h->dev.band_pad = (float)std::atof(e); }
  // lanes per query of the balanced listed search: round 4 measured it flat from 1 024 to 8 192 (3.13-3.25 ms per step), slower beyond
  // (16 384: 3.5, 32 768: 4.2); with the level-by-level row walk of round 5: 512 / 1 024 / 2 048 / 4 096 = +2.6 / +3.1 / +0.6 / 0 % alignments/s
  // on the bench batch together with 2 048 sums workgroups (one lane walks a short ball's few rows at no loss now).  At most kListedLaneBudgetMax: a pair's list is cut into at most budget / 256 + 1 items
  // (kListedMaxItems: finalize's segment table and the handle's seg_stride are sized for that)
  h->dev.listed_lane_budget = 1024;
  { const char* e = std::getenv("SMHIP_LISTED_LANES"); if (e && std::atoi(e) >= 256) h->dev.listed_lane_budget = std::min(std::atoi(e), kListedLaneBudgetMax); }
  h->split_share = 0.2f;
  { const char* e = std::getenv("SMHIP_SPLIT_SHARE"); if (e && std::atof(e) > 0.0) h->split_share = (float)std::atof(e); }
  h->sums_long_for = 3;
  { const char* e = std::getenv("SMHIP_SUMS_LONG_FOR"); if (e) h->sums_long_for = std::atoi(e); }
  h->use_shadow = 1;
  { const char* e = std::getenv("SMHIP_SHADOW"); if (e) h->use_shadow = std::atoi(e); }
  h->grid_sort_build = 1;
  { const char* e = std::getenv("SMHIP_GRID_BUILD"); if (e) h->grid_sort_build = std::atoi(e); }
  h->wave_search = 0;
  { const char* e = std::getenv("SMHIP_WAVE_SEARCH"); if (e) h->wave_search = std::atoi(e); }
  h->one_enabled = 1; h->one_blocks_want = 0;
  { const char* e = std::getenv("SMHIP_ONE_PAIR"); if (e) h->one_enabled = std::atoi(e); }
  { const char* e = std::getenv("SMHIP_ONE_BLOCKS"); if (e) h->one_blocks_want = std::atoi(e); }
  { const char* e = std::getenv("SMHIP_ONE_PAIRS"); h->one_pairs_max = e ? std::min(std::max(std::atoi(e), 1), kOnePairs) : kOnePairs; }
  h->one_idle = std::getenv("SMHIP_ONE_IDLE") != nullptr;
  h->one_no_retry = std::getenv("SMHIP_ONE_NO_RETRY") != nullptr;
  h->one_groups_want = 0;
  { const char* e = std::getenv("SMHIP_ONE_GROUPS"); if (e) h->one_groups_want = std::atoi(e); }
  h->sums_blocks = kSumsBlocks;
  { const char* e = std::getenv("SMHIP_SUMS_BLOCKS"); if (e && std::atoi(e) >= 8) h->sums_blocks = (std::min(std::atoi(e), 65536) / 8) * 8; }
  h->dev.listed_grain = 1;
  { const char* e = std::getenv("SMHIP_LISTED_GRAIN"); if (e && std::atoi(e) >= 0) h->dev.listed_grain = std::atoi(e); }
  { const char* e = std::getenv("SMHIP_BAND_GAIN"); if (e && std::atof(e) >= 0.0) h->dev.band_gain = (float)std::atof(e); }
  { const char* e = std::getenv("SMHIP_NABO_LISTED_BLOCKS"); if (e && std::atoi(e) > 0) h->nabo_listed_blocks = std::max(8, std::min(4096, std::atoi(e))); }   // >= 8: a workgroup's 16-bit histogram bins
}

// device CalculateNormals of n device rows (xyz in .x .y .z) into the target of `slot`; the workspace is there (prep_ensure)
smhip_status prep_run(smhip_context* h, const float4* raw_dev, int n, int slot, int* n_out) {
  // the leaf count is only known afterwards: run into the scratch halves of the staging-sized device buffer
  // when the slot's arrays could overflow, i.e. require nt_cap >= n / 4 + 8 (every leaf holds >= 4 points)
  if (h->dev.nt_cap < n / 4 + 8) { h->err = "max_target_points too small for the prepared target (need n / 4 + 8)"; return SMHIP_ERR_CAPACITY; }
  int m = 0;
  const hipError_t e = prep_calculate_normals(h->prep, h->stream, raw_dev, n,
                                              const_cast<float4*>(h->dev.tgt_p) + (size_t)slot * h->dev.nt_cap,
                                              const_cast<float4*>(h->dev.tgt_n) + (size_t)slot * h->dev.nt_cap, &m);
  // from here on the slot's target arrays have been written: whatever target it held is gone, also on the error paths
  touch_target(h, slot);
  h->nt[slot] = 0; h->has_normals[slot] = 0;
  if (e != hipSuccess) { h->err = std::string("prep_calculate_normals: ") + hipGetErrorString(e); return SMHIP_ERR_HIP; }
  if (m <= 0) { h->err = "CalculateNormals produced no target points"; return SMHIP_ERR_INVALID_ARGUMENT; }
  h->nt[slot] = m;
  h->has_normals[slot] = 1;
  touch_target(h, slot);
  if (n_out) *n_out = m;
  return SMHIP_OK;
}

}  // namespace smhip_host

namespace {

// FindClosests output in the caller's order: source i was uploaded from caller index src.w,
// target position j holds caller index tq.w.
__global__ void export_matches(IcpDev b, int pair, int32_t* out_ids, float* out_d2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= b.state[pair].ns) return;
  const int orig = __float_as_int(b.src[(size_t)pair * b.ns_cap + i].w);
  const int j = b.idx[(size_t)pair * b.ns_cap + i];
  out_ids[orig] = j < 0 ? -1 : __float_as_int(b.tq[(size_t)pair * b.nt_cap + j].w);
  out_d2[orig] = b.d2[(size_t)pair * b.ns_cap + i];
}

smhip_status fetch_matches(smhip_context* h, int slot, int32_t* ids, float* d2, int n) {
  if (n != h->ns[slot]) { h->err = "n must equal the slot's source size"; return SMHIP_ERR_INVALID_ARGUMENT; }
  hipLaunchKernelGGL(export_matches, dim3(ceil_div(n, 256)), dim3(256), 0, h->stream, h->dev, slot, h->ids_dev, h->d2_dev);
  HIPCHK(h, hipMemcpyAsync(h->ids_pinned, h->ids_dev, sizeof(int32_t) * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->d2_pinned, h->d2_dev, sizeof(float) * n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (ids) std::memcpy(ids, h->ids_pinned, sizeof(int32_t) * n);
  if (d2) std::memcpy(d2, h->d2_pinned, sizeof(float) * n);
  return SMHIP_OK;
}

}  // namespace

extern "C" {

int smhip_version(void) { return 100; }

const char* smhip_status_string(smhip_status s) {
  switch (s) {
    case SMHIP_OK: return "ok";
    case SMHIP_ERR_INVALID_ARGUMENT: return "invalid argument";
    case SMHIP_ERR_NO_DEVICE: return "no gfx950 device";
    case SMHIP_ERR_HIP: return "HIP runtime error";
    case SMHIP_ERR_NOT_READY: return "source/target not set";
    case SMHIP_ERR_NO_NORMALS: return "target has no normals";
    case SMHIP_ERR_NO_MATCH: return "no finite correspondence";
    case SMHIP_ERR_CAPACITY: return "cloud exceeds handle capacity";
    default: return "unknown";
  }
}

int smhip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -1;
  int good = 0;
  for (int i = 0; i < n; ++i) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, i) == hipSuccess && std::strncmp(p.gcnArchName, "gfx950", 6) == 0) ++good;
  }
  return good;
}

void smhip_icp_default_options(smhip_icp_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->max_iteration = 100;          // icp_fast.h:58
  o->dist_outlier_ratio = 0.7f;    // icp_fast.h:59
  o->early_exit = 1;
  o->nn_mode = SMHIP_NN_GRID;
  o->grid_cell = 0.25f;
  o->grid_max_ring = 8;
  o->check_every = 8;
  o->use_ball = 1;
  o->exact_matches = 0;
  o->ball_radius = 0.3f;
  o->ball_cap_factor = 1.5f;
  o->no_certify = 0;
  o->nn_epsilon = 3.16f;           // icp_fast.cc:174 (used by SMHIP_NN_NABO only)
}

smhip_status smhip_create(int device, void* stream, int pair_slots, int max_source_points, int max_target_points,
                          smhip_handle* out) {
  if (!out || pair_slots < 1 || max_source_points < 1 || max_target_points < 1) return SMHIP_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  const plan::Capacities cap = plan::plan_capacities(max_source_points);
  if (!cap.ok) return SMHIP_ERR_INVALID_ARGUMENT;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return SMHIP_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SMHIP_ERR_NO_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SMHIP_ERR_NO_DEVICE;   // gfx950-only code objects
  if (hipSetDevice(device) != hipSuccess) return SMHIP_ERR_NO_DEVICE;
  smhip_context* h = new smhip_context();
  h->device = device;
  if (stream) { h->stream = reinterpret_cast<hipStream_t>(stream); h->own_stream = false; }
  else {
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { delete h; return SMHIP_ERR_HIP; }
    h->own_stream = true;
  }
  if (hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess) h->ev_fork = nullptr;
  // side streams are created when a batch first asks for them (ensure_side_streams): the runtime maps streams onto a
  // handful of hardware queues (GPU_MAX_HW_QUEUES, default 4), so idle streams are not free
  smhip_icp_default_options(&h->opts);
  IcpDev& d = h->dev;
  d.slots = pair_slots; d.ns_cap = max_source_points; d.nt_cap = max_target_points;
  d.acc_blocks = cap.acc_blocks; d.part_stride = cap.part_stride; d.dl_stride = cap.dl_stride; d.bl_stride = cap.bl_stride; d.seg_stride = cap.seg_stride;
  d.acc_items = kAccItemsSmall;
  const size_t B = pair_slots, NS = max_source_points, NT = max_target_points;
  smhip_status s = SMHIP_OK;
  auto A = [&](smhip_status r) { if (s == SMHIP_OK) s = r; };
  A(dev_alloc(h, &d.state, B));
  A(dev_alloc(h, const_cast<PairInput**>(&d.in), B));
  A(dev_alloc(h, const_cast<float4**>(&d.src), B * NS));
  A(dev_alloc(h, const_cast<float**>(&d.src3), B * NS * 3));
  A(dev_alloc(h, const_cast<float4**>(&d.tgt_p), B * NT));
  A(dev_alloc(h, const_cast<float4**>(&d.tgt_n), B * NT));
  A(dev_alloc(h, &d.tq, B * NT));
  A(dev_alloc(h, &d.tn, B * NT));
  A(dev_alloc(h, &d.tcell, B * NT));
  A(dev_alloc(h, &d.tslot, B * NT));
  A(dev_alloc(h, &d.tord, B * NT));
  A(dev_alloc(h, &d.bits, B * kMaxGridWords));
  A(dev_alloc(h, &d.words, B * kMaxGridWords));
  A(dev_alloc(h, &d.rowbits, B * (size_t)kMaxRowWords));
  A(dev_alloc(h, &d.ccount, B * (NT + 1)));
  A(dev_alloc(h, &d.cstart, B * (NT + 1)));
  A(dev_alloc(h, &d.d2, B * NS));
  A(dev_alloc(h, &d.lb, B * NS));
  A(dev_alloc(h, &d.search_hist, B * kSearchHist));
  A(dev_alloc(h, &d.idx, B * NS));
  A(dev_alloc(h, &d.mb, B * NS));
  A(dev_alloc(h, &d.hist, B * kHistBins));
  A(dev_alloc(h, &d.dlist, B * (size_t)d.dl_stride));
  A(dev_alloc(h, &d.hlist, B * NS));
  A(dev_alloc(h, &d.ulist, B * NS));
  A(dev_alloc(h, &d.ukeys, B * NS));
  A(dev_alloc(h, &d.rec_a, B * 2 * (size_t)d.bl_stride));
  A(dev_alloc(h, &d.rec_j, B * 2 * (size_t)d.bl_stride));
  A(dev_alloc(h, &d.gcount, B * (size_t)d.seg_stride));
  A(dev_alloc(h, &d.dcount, B * (size_t)d.seg_stride));
  A(dev_alloc(h, &d.litems, B));
  A(dev_alloc(h, &d.partials, B * (size_t)d.part_stride * kAccCols));
  A(dev_alloc(h, &d.tpart, B * kTgtReduceBlocks * 16));
  A(dev_alloc(h, &d.done_count, 4));
  {   // everything of the single-pair cooperative launch that crosses workgroups: ONE fine-grained allocation (see IcpDev::one_ctr)
    const size_t w_sync = (size_t)kOneSyncWords * kOnePairs * 4, w_rows = (size_t)kOnePairs * (kOneMaxBlocks + 32) * kAccCols * 8,
                 w_hist = (size_t)kHistBins * kOnePairs * 4, w_keys = (size_t)kOnePairs * 2 * (size_t)d.bl_stride * 4, w_ctr = sizeof(PairState) * kOnePairs;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t total = up(w_sync) + up(w_rows) + up(w_hist) + up(w_keys) + up(w_ctr);
    void* v = nullptr;
    if (s == SMHIP_OK) {
      if (hipExtMallocWithFlags(&v, total, hipDeviceMallocFinegrained) != hipSuccess) {
        (void)hipGetLastError();
        v = nullptr;
        if (hipMalloc(&v, total) != hipSuccess) { s = SMHIP_ERR_HIP; v = nullptr; }
        h->one_blocks_allowed = 0;           // (no fine-grained memory: single pairs keep to the separate launches)
      }
      if (v) {
        h->allocs.push_back(v);
        char* c = reinterpret_cast<char*>(v);
        d.one_sync = reinterpret_cast<uint32_t*>(c); c += up(w_sync);
        d.one_rows = reinterpret_cast<double*>(c); c += up(w_rows);
        d.one_hist = reinterpret_cast<uint32_t*>(c); c += up(w_hist);
        d.one_keys = reinterpret_cast<uint32_t*>(c); c += up(w_keys);
        d.one_ctr = reinterpret_cast<PairState*>(c);
        if (hipMemsetAsync(v, 0, total, h->stream) != hipSuccess) s = SMHIP_ERR_HIP;
      }
    }
  }
  A(dev_alloc(h, &h->ids_dev, NS));
  A(dev_alloc(h, &h->d2_dev, NS));
  if (s == SMHIP_OK) {
    const size_t stage_n = 2 * std::max(NS, NT);
    if (hipHostMalloc(reinterpret_cast<void**>(&h->stage), stage_n * sizeof(float4)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&h->in_pinned), B * sizeof(PairInput)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&h->state_pinned), B * sizeof(PairState)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&h->done_pinned), 64) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&h->hist_pinned), B * kSearchHist * sizeof(uint32_t)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&h->ids_pinned), NS * sizeof(int32_t)) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&h->d2_pinned), NS * sizeof(float)) != hipSuccess)
      s = SMHIP_ERR_HIP;
  }
  if (s == SMHIP_OK) {
    // the single-pair persistent kernel meets at grid barriers: its grid is what the device holds at once (cooperative launch)
    int per_cu = 0, coop = 0;
    if (hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, device) == hipSuccess && coop &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, icp_one, kNnThreads, 0) == hipSuccess && per_cu > 0)
      h->one_blocks = (std::min(per_cu * prop.multiProcessorCount, kOneMaxBlocks) / 32) * 32;
    (void)hipGetLastError();
    if (!h->one_blocks_allowed) h->one_blocks = 0;
  }
  if (s == SMHIP_OK && hipMemsetAsync(d.state, 0, B * sizeof(PairState), h->stream) != hipSuccess) s = SMHIP_ERR_HIP;
  if (s == SMHIP_OK && hipStreamSynchronize(h->stream) != hipSuccess) s = SMHIP_ERR_HIP;
  if (s != SMHIP_OK) { smhip_destroy(h); return s; }
  h->ns.assign(B, 0); h->nt.assign(B, 0); h->has_normals.assign(B, 0);
  h->tgt_gen.assign(B, 0); h->grid_gen.assign(B, 0); h->src_gen.assign(B, 1); h->src3_gen.assign(B, 0); h->grid_cell_built.assign(B, 0.f); h->grid_sorted.assign(B, 0); h->grid_rows.assign(B, 0); h->grid_mode.assign(B, -1);
  sync_options(h);
  *out = h;
  return SMHIP_OK;
}

extern "C" void smhip_internal_free_ndt(smhip_context* h);
extern "C" void smhip_internal_free_gicp(smhip_context* h);
extern "C" void smhip_internal_free_m2dp(smhip_context* h);
extern "C" void smhip_internal_free_pose_graph(smhip_context* h);
extern "C" void smhip_internal_free_guess_search(smhip_context* h);

smhip_status smhip_destroy(smhip_handle h) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  smhip_internal_free_ndt(h);
  smhip_internal_free_gicp(h);
  smhip_internal_free_m2dp(h);
  smhip_internal_free_pose_graph(h);
  smhip_internal_free_guess_search(h);
  if (h->prep) prep_destroy(h->prep);
  if (h->prep_batch) prep_destroy(h->prep_batch);
  if (h->filt) filt_destroy(h->filt);
  for (void* p : h->allocs) (void)hipFree(p);
  if (h->stage) (void)hipHostFree(h->stage);
  if (h->in_pinned) (void)hipHostFree(h->in_pinned);
  if (h->state_pinned) (void)hipHostFree(h->state_pinned);
  if (h->done_pinned) (void)hipHostFree(h->done_pinned);
  if (h->hist_pinned) (void)hipHostFree(h->hist_pinned);
  if (h->ids_pinned) (void)hipHostFree(h->ids_pinned);
  if (h->d2_pinned) (void)hipHostFree(h->d2_pinned);
  for (auto& e : h->ev_pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (int k = 0; k < h->n_side; ++k) {
    (void)hipStreamSynchronize(h->side[k]); (void)hipStreamDestroy(h->side[k]); (void)hipEventDestroy(h->ev_join[k]);
  }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->copy_stream) { (void)hipStreamSynchronize(h->copy_stream); (void)hipStreamDestroy(h->copy_stream); }
  if (h->ev_copied) (void)hipEventDestroy(h->ev_copied);
  if (h->ev_raw_free) (void)hipEventDestroy(h->ev_raw_free);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return SMHIP_OK;
}

const char* smhip_last_error(smhip_handle h) { return h ? h->err.c_str() : "null handle"; }

smhip_status smhip_icp_set_options(smhip_handle h, const smhip_icp_options* o) {
  if (!h || !o) return SMHIP_ERR_INVALID_ARGUMENT;
  if (!(o->dist_outlier_ratio >= 0.f && o->dist_outlier_ratio <= 1.f)) {     // icp_fast.cc:68 CHECK
    h->err = "dist_outlier_ratio must be in [0, 1]";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  if (o->nn_mode != SMHIP_NN_BRUTE && o->nn_mode != SMHIP_NN_GRID && o->nn_mode != SMHIP_NN_NABO) { h->err = "bad nn_mode"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (o->nn_mode == SMHIP_NN_NABO && !(o->nn_epsilon >= 0.f)) { h->err = "nn_epsilon must be >= 0"; return SMHIP_ERR_INVALID_ARGUMENT; }
  h->opts = *o;
  if (h->opts.check_every < 1) h->opts.check_every = 8;
  sync_options(h);
  if (o->nn_mode == SMHIP_NN_NABO) {      // the mode's arrays (tree, work classes) are allocated here, never inside Align
    HIPCHK(h, hipSetDevice(h->device));
    return kd_ensure(h);
  }
  return SMHIP_OK;
}

smhip_status smhip_synchronize(smhip_handle h) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return SMHIP_OK;
}

// ---- uploads ---------------------------------------------------------------------------

// staged source -> device, Morton-ordered there (spatially coherent wavefronts; w = caller index)
static smhip_status upload_source(smhip_handle h, int slot, int n) {
  smhip_status s = prep_ensure(h);
  if (s) return s;
  HIPCHK(h, hipMemcpyAsync(h->prep_raw, h->stage, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  const hipError_t e = prep_morton_sort(h->prep, h->stream, h->prep_raw, n, const_cast<float4*>(h->dev.src) + (size_t)slot * h->dev.ns_cap);
  if (e != hipSuccess) { h->err = std::string("prep_morton_sort: ") + hipGetErrorString(e); return SMHIP_ERR_HIP; }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->ns[slot] = n;
  touch_source(h, slot);
  return SMHIP_OK;
}

static smhip_status upload(smhip_handle h, const float4* dst_dev, const float4* staged, int n) {
  HIPCHK(h, hipMemcpyAsync(const_cast<float4*>(dst_dev), staged, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  return SMHIP_OK;
}

smhip_status smhip_set_source_f64(smhip_handle h, int slot, const double* xyz, int n) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!xyz || n <= 0) { h->err = "empty source cloud"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (n > h->dev.ns_cap) { h->err = "source larger than max_source_points"; return SMHIP_ERR_CAPACITY; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // staging buffer reuse
  for (int i = 0; i < n; ++i) h->stage[i] = make_float4((float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2], 0.f);
  return upload_source(h, slot, n);
}

smhip_status smhip_set_source_f32(smhip_handle h, int slot, const float* xyz, int stride, int n) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!xyz || n <= 0 || stride < 3) { h->err = "empty source cloud / bad stride"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (n > h->dev.ns_cap) { h->err = "source larger than max_source_points"; return SMHIP_ERR_CAPACITY; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (stride == 4) std::memcpy(h->stage, xyz, sizeof(float4) * (size_t)n);      // KITTI rows are already float4 (w is overwritten on the device)
  else for (int i = 0; i < n; ++i) h->stage[i] = make_float4(xyz[(size_t)stride * i], xyz[(size_t)stride * i + 1], xyz[(size_t)stride * i + 2], 0.f);
  return upload_source(h, slot, n);
}

smhip_status smhip_reserve_batch_workspaces(smhip_handle h) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->prep_batch) {
    h->prep_batch = prep_create(h->dev.slots * h->dev.ns_cap);
    if (!h->prep_batch) { h->err = "batch workspace allocation failed"; return SMHIP_ERR_HIP; }
  }
  if (prep_reserve_forest(h->prep_batch) != hipSuccess) { h->err = "batch workspace allocation failed (CalculateNormals forest)"; return SMHIP_ERR_HIP; }
  if (!h->raw_batch) {
    smhip_status s = dev_alloc(h, &h->raw_batch, (size_t)h->dev.slots * h->dev.ns_cap);
    if (s) return s;
  }
  return SMHIP_OK;
}

smhip_status smhip_set_sources_f32_batch(smhip_handle h, int count, const int* slots, const float* const* rows, const int* n) {
  if (!h || !slots || !rows || !n || count < 1 || count > h->dev.slots || count > 512) { if (h) h->err = "bad batch of sources"; return SMHIP_ERR_INVALID_ARGUMENT; }
  long long total = 0;
  for (int k = 0; k < count; ++k) {
    smhip_status s = check_slot(h, slots[k]);
    if (s) return s;
    if (!rows[k] || n[k] <= 0) { h->err = "empty source cloud"; return SMHIP_ERR_INVALID_ARGUMENT; }
    if (n[k] > h->dev.ns_cap) { h->err = "source larger than max_source_points"; return SMHIP_ERR_CAPACITY; }
    total += n[k];
  }
  if (total > 0x7fffffffll) { h->err = "batch of sources holds more than 2^31 points (the staging offsets are 32-bit)"; return SMHIP_ERR_CAPACITY; }
  HIPCHK(h, hipSetDevice(h->device));
  if (!h->prep_batch) {
    h->prep_batch = prep_create(h->dev.slots * h->dev.ns_cap);
    if (!h->prep_batch) { h->err = "batched upload workspace allocation failed"; return SMHIP_ERR_HIP; }
  }
  if (!h->raw_batch) {
    smhip_status s = dev_alloc(h, &h->raw_batch, (size_t)h->dev.slots * h->dev.ns_cap);
    if (s) return s;
  }
  // rows -> the device staging array, cloud after cloud.  Pinned rows are copied from where they lie (no host copy, the call
  // returns at once); pageable rows go through the handle's one pinned buffer, which must have left the host before it is
  // filled again.
  std::vector<int> stage_off(count);
  std::vector<long long> out_off(count);
  std::vector<char> is_pinned(count);
  bool all_pinned = true;
  for (int k = 0; k < count; ++k) {
    hipPointerAttribute_t attr{};
    is_pinned[k] = hipPointerGetAttributes(&attr, rows[k]) == hipSuccess && attr.type == hipMemoryTypeHost;
    if (!is_pinned[k]) { (void)hipGetLastError(); all_pinned = false; }
  }
  // All rows page-locked: the copies go to a stream of their own, so the DMA engines bring the next batch in while the
  // handle's stream is still aligning the previous one (a batch of 256 scans is 0.5 GB: 10 ms of a 50 ms batch).  The staging
  // array is free once the previous batch's Morton ordering has read it (ev_raw_free), and the ordering of this batch waits
  // for the copies (ev_copied).
  hipStream_t cs = h->stream;
  if (all_pinned) {
    if (!h->copy_stream) {
      if (hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&h->ev_copied, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&h->ev_raw_free, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); h->copy_stream = nullptr; }
    }
    if (h->copy_stream) {
      cs = h->copy_stream;
      if (h->raw_in_use) HIPCHK(h, hipStreamWaitEvent(cs, h->ev_raw_free, 0));
    }
  }
  long long at = 0;
  for (int k = 0; k < count; ++k) {
    stage_off[k] = (int)at;
    out_off[k] = (long long)slots[k] * h->dev.ns_cap;
    const void* from = rows[k];
    if (!is_pinned[k]) {
      HIPCHK(h, hipStreamSynchronize(h->stream));
      std::memcpy(h->stage, rows[k], sizeof(float4) * (size_t)n[k]);
      from = h->stage;
    }
    HIPCHK(h, hipMemcpyAsync(h->raw_batch + at, from, sizeof(float4) * (size_t)n[k], hipMemcpyHostToDevice, cs));
    at += n[k];
  }
  if (cs != h->stream) {
    HIPCHK(h, hipEventRecord(h->ev_copied, cs));
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_copied, 0));
  }
  const hipError_t e = prep_morton_sort_batch(h->prep_batch, h->stream, h->raw_batch, count, stage_off.data(), n, out_off.data(), const_cast<float4*>(h->dev.src));
  if (e != hipSuccess) { h->err = std::string("prep_morton_sort_batch: ") + hipGetErrorString(e); return SMHIP_ERR_HIP; }
  if (h->ev_raw_free) { HIPCHK(h, hipEventRecord(h->ev_raw_free, h->stream)); h->raw_in_use = true; }
  for (int k = 0; k < count; ++k) { h->ns[slots[k]] = n[k]; touch_source(h, slots[k]); }
  return SMHIP_OK;
}

smhip_status smhip_set_target_f64(smhip_handle h, int slot, const double* xyz, const double* nrm, int n) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!xyz || n <= 0) { h->err = "empty target cloud"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (n > h->dev.nt_cap) { h->err = "target larger than max_target_points"; return SMHIP_ERR_CAPACITY; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float4* sp = h->stage;
  float4* sn = h->stage + std::max(h->dev.ns_cap, h->dev.nt_cap);
  bool finite = true;
  for (int i = 0; i < n; ++i) {
    sp[i] = make_float4((float)xyz[3 * i], (float)xyz[3 * i + 1], (float)xyz[3 * i + 2], 0.f);
    sn[i] = nrm ? make_float4((float)nrm[3 * i], (float)nrm[3 * i + 1], (float)nrm[3 * i + 2], 0.f) : make_float4(0, 0, 0, 0);
    finite = finite && std::isfinite(sp[i].x) && std::isfinite(sp[i].y) && std::isfinite(sp[i].z);
  }
  if (!finite) { h->err = "target cloud has NaN / Inf coordinates"; return SMHIP_ERR_INVALID_ARGUMENT; }
  s = upload(h, h->dev.tgt_p + (size_t)slot * h->dev.nt_cap, sp, n);
  if (s) return s;
  s = upload(h, h->dev.tgt_n + (size_t)slot * h->dev.nt_cap, sn, n);
  if (s) return s;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->nt[slot] = n;
  h->has_normals[slot] = nrm != nullptr;
  touch_target(h, slot);
  return SMHIP_OK;
}

smhip_status smhip_set_target_f32(smhip_handle h, int slot, const float* xyz, int stride, const float* nrm, int nstride, int n) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!xyz || n <= 0 || stride < 3 || (nrm && nstride < 3)) { h->err = "empty target cloud / bad stride"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (n > h->dev.nt_cap) { h->err = "target larger than max_target_points"; return SMHIP_ERR_CAPACITY; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float4* sp = h->stage;
  float4* sn = h->stage + std::max(h->dev.ns_cap, h->dev.nt_cap);
  bool finite = true;
  for (int i = 0; i < n; ++i) {
    sp[i] = make_float4(xyz[(size_t)stride * i], xyz[(size_t)stride * i + 1], xyz[(size_t)stride * i + 2], 0.f);
    sn[i] = nrm ? make_float4(nrm[(size_t)nstride * i], nrm[(size_t)nstride * i + 1], nrm[(size_t)nstride * i + 2], 0.f) : make_float4(0, 0, 0, 0);
    finite = finite && std::isfinite(sp[i].x) && std::isfinite(sp[i].y) && std::isfinite(sp[i].z);
  }
  if (!finite) { h->err = "target cloud has NaN / Inf coordinates"; return SMHIP_ERR_INVALID_ARGUMENT; }
  s = upload(h, h->dev.tgt_p + (size_t)slot * h->dev.nt_cap, sp, n);
  if (s) return s;
  s = upload(h, h->dev.tgt_n + (size_t)slot * h->dev.nt_cap, sn, n);
  if (s) return s;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->nt[slot] = n;
  h->has_normals[slot] = nrm != nullptr;
  touch_target(h, slot);
  return SMHIP_OK;
}

smhip_status smhip_prepare_target_f32(smhip_handle h, int slot, const float* xyz, int stride, int n, int* n_out) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!xyz || n <= 0 || stride < 3) { h->err = "empty cloud / bad stride"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (n > std::max(h->dev.ns_cap, h->dev.nt_cap)) { h->err = "scan larger than the handle's capacity"; return SMHIP_ERR_CAPACITY; }
  HIPCHK(h, hipSetDevice(h->device));
  s = prep_ensure(h);
  if (s) return s;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (stride == 4) std::memcpy(h->stage, xyz, sizeof(float4) * (size_t)n);
  else for (int i = 0; i < n; ++i) h->stage[i] = make_float4(xyz[(size_t)stride * i], xyz[(size_t)stride * i + 1], xyz[(size_t)stride * i + 2], 0.f);
  HIPCHK(h, hipMemcpyAsync(h->prep_raw, h->stage, sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  return prep_run(h, h->prep_raw, n, slot, n_out);
}

smhip_status smhip_prepare_target_from_source(smhip_handle h, int from, int to, int* n_out) {
  smhip_status s = check_slot(h, from);
  if (s) return s;
  s = check_slot(h, to);
  if (s) return s;
  if (h->ns[from] <= 0) { h->err = "source slot is empty"; return SMHIP_ERR_NOT_READY; }
  HIPCHK(h, hipSetDevice(h->device));
  s = prep_ensure(h);
  if (s) return s;
  return prep_run(h, h->dev.src + (size_t)from * h->dev.ns_cap, h->ns[from], to, n_out);
}

smhip_status smhip_prepare_targets_from_sources(smhip_handle h, int count, const int* from_slots, const int* to_slots, int* n_out) {
  if (!h || !from_slots || !to_slots || count < 1 || count > h->dev.slots) return SMHIP_ERR_INVALID_ARGUMENT;
  HIPCHK(h, hipSetDevice(h->device));
  std::vector<int> off(count), n(count), out_off(count), m(count, 0);
  for (int k = 0; k < count; ++k) {
    smhip_status s = check_slot(h, from_slots[k]);
    if (s) return s;
    s = check_slot(h, to_slots[k]);
    if (s) return s;
    if (h->ns[from_slots[k]] <= 0) { h->err = "source slot is empty"; return SMHIP_ERR_NOT_READY; }
    n[k] = h->ns[from_slots[k]];
    if (h->dev.nt_cap < n[k] / 4 + 8) { h->err = "max_target_points too small for the prepared target (need n / 4 + 8)"; return SMHIP_ERR_CAPACITY; }
    off[k] = from_slots[k] * h->dev.ns_cap;
    out_off[k] = to_slots[k] * h->dev.nt_cap;
  }
  if (!h->prep_batch) {
    h->prep_batch = prep_create(h->dev.slots * h->dev.ns_cap);
    if (!h->prep_batch) { h->err = "batched CalculateNormals workspace allocation failed"; return SMHIP_ERR_HIP; }
  }
  const hipError_t e = prep_calculate_normals_batch(h->prep_batch, h->stream, h->dev.src, count, off.data(), n.data(), out_off.data(),
                                                    const_cast<float4*>(h->dev.tgt_p), const_cast<float4*>(h->dev.tgt_n), m.data());
  for (int k = 0; k < count; ++k) { touch_target(h, to_slots[k]); h->nt[to_slots[k]] = 0; h->has_normals[to_slots[k]] = 0; }   // overwritten, whatever follows
  if (e != hipSuccess) { h->err = std::string("prep_calculate_normals_batch: ") + hipGetErrorString(e); return SMHIP_ERR_HIP; }
  for (int k = 0; k < count; ++k) {
    if (m[k] <= 0) { h->err = "CalculateNormals produced no target points"; return SMHIP_ERR_INVALID_ARGUMENT; }
    h->nt[to_slots[k]] = m[k];
    h->has_normals[to_slots[k]] = 1;
    touch_target(h, to_slots[k]);
    if (n_out) n_out[k] = m[k];
  }
  return SMHIP_OK;
}

smhip_status smhip_prepare_target_from_target(smhip_handle h, int from, int to, int* n_out) {
  smhip_status s = check_slot(h, from);
  if (s) return s;
  s = check_slot(h, to);
  if (s) return s;
  if (from == to) { h->err = "from_slot == to_slot: the raw target would be overwritten while it is read"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (h->nt[from] <= 0) { h->err = "target slot is empty"; return SMHIP_ERR_NOT_READY; }
  HIPCHK(h, hipSetDevice(h->device));
  s = prep_ensure(h);
  if (s) return s;
  return prep_run(h, h->dev.tgt_p + (size_t)from * h->dev.nt_cap, h->nt[from], to, n_out);
}

smhip_status smhip_sample_source(smhip_handle h, int from, int to, float prob, uint32_t seed, int* n_out) {
  smhip_status s = check_slot(h, from);
  if (s) return s;
  s = check_slot(h, to);
  if (s) return s;
  if (from == to) { h->err = "from_slot == to_slot"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (h->ns[from] <= 0) { h->err = "source slot is empty"; return SMHIP_ERR_NOT_READY; }
  if (!(prob > 0.f)) { h->err = "sampling probability must be > 0"; return SMHIP_ERR_INVALID_ARGUMENT; }
  HIPCHK(h, hipSetDevice(h->device));
  s = prep_ensure(h);
  if (s) return s;
  int m = 0;
  const hipError_t e = prep_sample_morton(h->prep, h->stream, h->dev.src + (size_t)from * h->dev.ns_cap, h->ns[from], prob, seed,
                                          const_cast<float4*>(h->dev.src) + (size_t)to * h->dev.ns_cap, &m);
  if (e != hipSuccess) { h->err = std::string("prep_sample_morton: ") + hipGetErrorString(e); return SMHIP_ERR_HIP; }
  if (m <= 0) { h->err = "sampling kept no point"; return SMHIP_ERR_INVALID_ARGUMENT; }
  h->ns[to] = m;
  touch_source(h, to);
  if (n_out) *n_out = m;
  return SMHIP_OK;
}

smhip_status smhip_get_target_f32(smhip_handle h, int slot, float* xyz, float* normals, int n) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (n != h->nt[slot] || n <= 0) { h->err = "n must equal the slot's target size"; return SMHIP_ERR_INVALID_ARGUMENT; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  float4* sp = h->stage;
  float4* sn = h->stage + std::max(h->dev.ns_cap, h->dev.nt_cap);
  HIPCHK(h, hipMemcpyAsync(sp, h->dev.tgt_p + (size_t)slot * h->dev.nt_cap, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(sn, h->dev.tgt_n + (size_t)slot * h->dev.nt_cap, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < n; ++i) {
    if (xyz) { xyz[3 * i] = sp[i].x; xyz[3 * i + 1] = sp[i].y; xyz[3 * i + 2] = sp[i].z; }
    if (normals) { normals[3 * i] = sn[i].x; normals[3 * i + 1] = sn[i].y; normals[3 * i + 2] = sn[i].z; }
  }
  return SMHIP_OK;
}

smhip_status smhip_get_source_f32(smhip_handle h, int slot, float* xyzw, int n) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!xyzw || n != h->ns[slot] || n <= 0) { h->err = "n must equal the slot's source size"; return SMHIP_ERR_INVALID_ARGUMENT; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpyAsync(h->stage, h->dev.src + (size_t)slot * h->dev.ns_cap, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  std::memcpy(xyzw, h->stage, sizeof(float4) * (size_t)n);
  return SMHIP_OK;
}

smhip_status smhip_copy_slot(smhip_handle h, int from, int to) {
  smhip_status s = check_slot(h, from);
  if (s) return s;
  s = check_slot(h, to);
  if (s) return s;
  if (from == to) return SMHIP_OK;
  HIPCHK(h, hipSetDevice(h->device));
  IcpDev& d = h->dev;
  hipLaunchKernelGGL(copy_slot, dim3(ceil_div(std::max(d.ns_cap, d.nt_cap), 256)), dim3(256), 0, h->stream, d,
                     const_cast<float4*>(d.src), const_cast<float4*>(d.tgt_p), const_cast<float4*>(d.tgt_n), from, to);
  HIPCHK(h, hipGetLastError());
  h->ns[to] = h->ns[from]; h->nt[to] = h->nt[from]; h->has_normals[to] = h->has_normals[from];
  touch_source(h, to);
  touch_target(h, to);
  return SMHIP_OK;
}

// fewer side streams than asked for = less overlap, still correct
static void ensure_side_streams(smhip_context* h, int n) {
  if (!h->ev_fork) return;
  for (int k = h->n_side; k < n && k < plan::kMaxParts - 1; ++k) {
    if (hipStreamCreateWithFlags(&h->side[k], hipStreamNonBlocking) != hipSuccess) { h->side[k] = nullptr; return; }
    if (hipEventCreateWithFlags(&h->ev_join[k], hipEventDisableTiming) != hipSuccess) { (void)hipStreamDestroy(h->side[k]); h->side[k] = nullptr; return; }
    h->n_side = k + 1;
  }
}

// ---- Align -------------------------------------------------------------------------------
static smhip_status enqueue_range(smhip_handle h, int first, int npairs, const double* guesses) {
  if (!h || !guesses || npairs < 1 || first < 0 || first + npairs > h->dev.slots) {
    if (h) h->err = "bad slot range / guesses";
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  // inner compensation is defined over the grid search alone (the reference-search and brute modes are out of its scope): refused
  // before anything is touched
  if (h->inner_comp && h->opts.nn_mode != SMHIP_NN_GRID) { h->err = "inner compensation runs with nn_mode SMHIP_NN_GRID only"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (h->inner_comp && !h->dev.comp3) { h->err = "inner compensation: the step cloud's array is missing (internal)"; return SMHIP_ERR_NOT_READY; }
  HIPCHK(h, hipSetDevice(h->device));
  int ns_max = 0, nt_max = 0;
  // in_pinned may still be in flight from a previous enqueue on this stream
  HIPCHK(h, hipStreamSynchronize(h->stream));
  smhip_status s = fill_inputs(h, npairs, guesses, &ns_max, &nt_max, first);
  if (s) return s;
  if (h->hist_pairs > 0) {
    // the previous batch is complete (stream synchronised above): its searched shares place this one's switch to the two-launch form
    const int k = plan::split_from_history(h->hist_pinned, h->hist_ns.data(), h->hist_pairs, h->hist_iters, h->split_share);
    if (h->hist_mode == SMHIP_NN_NABO) h->nabo_fused_from = plan::clamp_split(k, plan::kNaboFusedFromMax);
    else h->auto_split = plan::clamp_split(k, plan::kAutoSplitMax);
    h->hist_pairs = 0;
  }
  if (h->opts.split_after == 0) h->dev.split_after = h->auto_split;
  const bool cached_one = npairs == 1 && grid_cached(h, first);
  if (cached_one) s = enqueue_prepare_one(h, first, nt_max);     // target unchanged: pose + scratch reset only
  else s = enqueue_resets(h, npairs, first, nt_max);
  if (s) return s;
  // Split the batch over several streams: the latency-bound launches of one part (finalize, validate, grid
  // build, near-empty refinement kernels) overlap the throughput-bound NN / accumulate of the others.
  plan::Inputs in = plan_inputs(h);
  if (const int want = plan::parts_wanted(in, npairs); want > 1) { ensure_side_streams(h, want - 1); in.side_streams = h->n_side; }
  const plan::Batch batch = plan::plan_batch(in, npairs, ns_max, nt_max);
  h->prof.split_after_used = batch.split_after_used;
  Half halves[plan::kMaxParts];
  const int nh = batch.nparts;
  for (int k = 0; k < nh; ++k) {
    const plan::Part& p = batch.part[k];
    halves[k] = whole_batch(h, p.np, first + p.first);
    halves[k].stream = k == 0 ? h->stream : h->side[k - 1];
    halves[k].part = p;
    halves[k].part.nt_max = nt_max_of(h, first + p.first, p.np);
    halves[k].d.acc_items = p.acc_items;
    if (in.compensation) {
      // the iteration kernels of this Align stream the step cloud comp_apply writes (IcpDev goes by value: the slot's own src3 is
      // neither moved nor overwritten) and search every query: no certificate survives a step that is not rigid
      halves[k].d.src3 = h->dev.comp3;
      halves[k].d.certify = 0;
    }
  }
  auto fork = [&]() -> smhip_status {
    if (nh > 1) {
      HIPCHK(h, hipEventRecord(h->ev_fork, h->stream));
      for (int k = 1; k < nh; ++k) HIPCHK(h, hipStreamWaitEvent(h->side[k - 1], h->ev_fork, 0));
    }
    return SMHIP_OK;
  };
  auto join = [&]() -> smhip_status {
    for (int k = 1; k < nh; ++k) {
      HIPCHK(h, hipEventRecord(h->ev_join[k - 1], h->side[k - 1]));
      HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_join[k - 1], 0));
    }
    return SMHIP_OK;
  };
  s = fork();
  if (s) return s;
  const int max_it = h->dev.max_iteration;
  bool grid_built = false;
  h->one_used = 0;
  if (batch.one_launch) {      // the whole loop and the score as ONE cooperative launch (plan_batch)
    if (!cached_one) { s = enqueue_grid_build(h, halves[0], nt_max); if (s) return s; }
    grid_built = true;
    IcpDev d1 = halves[0].d;
    d1.fused = 0; d1.fused_nabo = 0;
    int groups = batch.one_groups;
    void* args[] = {&d1, &groups};
    if (hipLaunchCooperativeKernel(reinterpret_cast<const void*>(icp_one), dim3(batch.one_grid, npairs), dim3(kNnThreads), args, 0, h->stream) == hipSuccess) {
      h->one_used = 1;
      h->one_launches += 1;
      h->last_npairs = npairs;
      return SMHIP_OK;
    }
    // the runtime refused the cooperative launch (it cannot place the grid): not an error of the Align -- the same iterations as
    // separate launches below, and no further attempts on this handle
    (void)hipGetLastError();
    h->one_blocks = 0;
  }
  // one iteration of one part: FindClosests, the sums, finalize
  auto enqueue_iteration = [&](Half& f, int it) -> smhip_status {
    const plan::Iteration p = plan::plan_iteration(in, f.part, ns_max, it, f.first_fused);
    f.first_fused = p.first_fused;
    f.d.fused = p.fused; f.d.fused_nabo = p.fused_nabo; f.d.sums_items = p.sums_items;
    return enqueue_launches(h, f, p);
  };
  // (The parts march in lock-step.  Tried in round 5: part k + 1 started two to five iterations behind part k, so that one part's
  // searching iterations -- bound by vector-instruction issue -- would run beside another's streaming ones -- bound by HBM: no gain
  // with 2, 3, 4 or 8 parts (24.0 / 23.9 / 23.5 / 18.7 k alignments/s against 24.4 k in lock-step).  Side by side the two kernels
  // split the registers: the certificate pass needs all of its waves to keep ~10 MB in flight, the search all of its to fill the
  // SIMDs, and each runs as much slower as the other gains.)
  if (!cached_one && !grid_built) for (int k = 0; k < nh; ++k) { s = enqueue_grid_build(h, halves[k], nt_max); if (s) return s; }
  for (int it = 0; it < max_it; ++it) {
    for (int k = 0; k < nh; ++k) {
      s = enqueue_iteration(halves[k], it);
      if (s) return s;
    }
    if (h->dev.early_exit && (it + 1) % h->opts.check_every == 0 && it + 1 < max_it) {
      s = join();
      if (s) return s;
      HIPCHK(h, hipMemcpyAsync(h->done_pinned, h->dev.done_count, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (*h->done_pinned >= (uint32_t)npairs) break;
      s = fork();      // re-fork for the next chunk of iterations
      if (s) return s;
    }
  }
  // the score of the iteration every pair left the loop with (icp_fast.cc:516-522), from that iteration's distances
  for (int k = 0; k < nh; ++k) {
    Half& f = halves[k];
    Bracket br(h, plan::kCatSolve, f.stream);
    hipLaunchKernelGGL(final_score, dim3(f.np * kScoreParts), dim3(kAccThreads), 0, f.stream, f.d);
    hipLaunchKernelGGL(score_fold, dim3(ceil_div(f.np, 256)), dim3(256), 0, f.stream, f.d, f.np);
  }
  s = join();
  if (s) return s;
  if (batch.record_history) {
    h->hist_mode = h->opts.nn_mode;
    HIPCHK(h, hipMemcpyAsync(h->hist_pinned, h->dev.search_hist + (size_t)first * kSearchHist, sizeof(uint32_t) * kSearchHist * (size_t)npairs,
                             hipMemcpyDeviceToHost, h->stream));
    h->hist_first = first; h->hist_pairs = npairs; h->hist_iters = max_it;
    h->hist_ns.assign(h->ns.begin() + first, h->ns.begin() + first + npairs);
  }
  HIPCHK(h, hipGetLastError());
  h->last_npairs = npairs;
  return SMHIP_OK;
}

smhip_status smhip_icp_enqueue_batch(smhip_handle h, int npairs, const double* guesses) { return enqueue_range(h, 0, npairs, guesses); }

static smhip_status fetch_range(smhip_handle h, int first, int npairs, double* results, double* scores, smhip_icp_stats* stats) {
  if (!h || npairs < 1 || first < 0 || first + npairs > h->dev.slots) return SMHIP_ERR_INVALID_ARGUMENT;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(h->state_pinned, h->dev.state + first, sizeof(PairState) * npairs, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->one_used && !h->one_no_retry) {
    // The cooperative launch stopped itself (its barrier watchdog or its workgroups' consistency check, icp_one.hip): never seen
    // on a single pair, but the protocol rests on the timing of agent-scope loads, not on fences -- so the Align is simply done
    // again as separate launches (whose result differs from the launch's in the sums' order: ~1e-15) and the handle keeps to them.
    bool stopped = false;
    for (int p = 0; p < npairs; ++p)
      stopped = stopped || (h->state_pinned[p].done && (h->state_pinned[p].status == SMHIP_ERR_HIP || (h->state_pinned[p].status == SMHIP_OK && h->state_pinned[p].score_mismatch)));
    if (stopped) {
      std::vector<double> g(16 * (size_t)npairs);
      for (int p = 0; p < npairs; ++p)
        for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) g[16 * (size_t)p + 4 * c + r] = h->in_pinned[first + p].guess[4 * r + c];
      h->one_blocks = 0;
      h->one_fallbacks += 1;
      const smhip_status rs = enqueue_range(h, first, npairs, g.data());
      if (rs) return rs;
      HIPCHK(h, hipMemcpyAsync(h->state_pinned, h->dev.state + first, sizeof(PairState) * npairs, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
  }
  collect_profile(h);
  smhip_status worst = SMHIP_OK;
  for (int p = 0; p < npairs; ++p) {
    const PairState& st = h->state_pinned[p];
    if (results) std::memcpy(results + 16 * p, st.result, sizeof(double) * 16);
    if (scores) scores[p] = st.score;
    if (stats) {
      stats[p].iterations = st.iter;
      stats[p].kept = st.kept;
      float lim; uint32_t key = st.limit_key; std::memcpy(&lim, &key, 4);
      stats[p].limit_d2 = lim;
      stats[p].fallback_queries = (int32_t)st.fallback_total;
      stats[p].status = st.status;
      stats[p].hard_queries = (int32_t)st.hard_total;
      stats[p].refined_iterations = (int32_t)st.refine_total;
      stats[p].searched_queries = (int32_t)st.searched_total;
      stats[p].fused_iterations = (int32_t)st.spec_hits;
    }
    if (st.status != SMHIP_OK && worst == SMHIP_OK) {
      worst = st.status;
      h->err = st.status == SMHIP_ERR_INVALID_ARGUMENT ? "pair failed: target cloud has NaN / Inf coordinates"
             : (st.status == SMHIP_ERR_HIP ? "pair failed: the single-pair launch stopped itself (a grid barrier did not complete, or its workgroups disagreed; internal)" : "pair failed: no finite correspondence");
      if (st.status == SMHIP_ERR_HIP && h->one_used) {
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        (void)hipMemcpy(w, h->dev.one_sync + (size_t)p * kOneSyncWords + kSyncAbort, sizeof(w), hipMemcpyDeviceToHost);
        char buf[256];
        if (w[0] == 2u)
          std::snprintf(buf, sizeof(buf), " [pair %d: workgroups disagree -- workgroup %u at barrier %u has quantile key %u / %u distances, column %u averages %u]", p, w[1], w[2], w[3], w[4], w[5], w[6]);
        else
          std::snprintf(buf, sizeof(buf), " [pair %d: noticed by workgroup %u at barrier %u: group arrivals %u of %u, groups arrived %u of %u]", p, w[1], w[2], w[3], w[4], w[5], w[6]);
        h->err += buf;
#if SMHIP_ONE_CHECKS
        {   // (diagnostic build) the barriers every workgroup entered, in order: where do they part?
          const int G = 64, N = 64;
          std::vector<uint32_t> tr((size_t)G * N * 4);
          (void)hipMemcpy(tr.data(), h->dev.rec_a + (size_t)p * 2 * h->dev.bl_stride, tr.size() * 4, hipMemcpyDeviceToHost);
          for (int n = 0; n < N; ++n) {
            bool same = true;
            for (int w = 1; w < 40; ++w) for (int c = 0; c < 3; ++c) same = same && tr[((size_t)w * N + n) * 4 + c] == tr[(size_t)n * 4 + c];
            if (!same) {
              std::fprintf(stderr, "[icp_one trace] pair %d: workgroups part at their barrier %d:", p, n + 1);
              for (int w = 0; w < 40; ++w) std::fprintf(stderr, " %u/%u/%u/%u", tr[((size_t)w * N + n) * 4], tr[((size_t)w * N + n) * 4 + 1], tr[((size_t)w * N + n) * 4 + 2], tr[((size_t)w * N + n) * 4 + 3]);
              std::fprintf(stderr, "\n");
              break;
            }
          }
        }
#endif
      }
    }
    if (!st.done && worst == SMHIP_OK) { worst = SMHIP_ERR_HIP; h->err = "pair did not finish (internal)"; }
    if (st.done && st.status == SMHIP_OK && st.score_mismatch && worst == SMHIP_OK) {
      worst = SMHIP_ERR_HIP; h->err = "score: the matches summed are not the matches finalize kept (internal)";
      char buf[160];
      std::snprintf(buf, sizeof(buf), " [pair %d: %u distances at or below the quantile, %d kept by the last iteration (%d iterations, %u fused)]", p, st.score_cnt[0], st.kept, st.iter, st.spec_hits);
      h->err += buf;
    }
  }
  return worst;
}

smhip_status smhip_icp_fetch_batch(smhip_handle h, int npairs, double* results, double* scores, smhip_icp_stats* stats) {
  return fetch_range(h, 0, npairs, results, scores, stats);
}

smhip_status smhip_icp_align_range(smhip_handle h, int first_slot, int npairs, const double* guesses, double* results,
                                   double* scores, smhip_icp_stats* stats) {
  smhip_status s = enqueue_range(h, first_slot, npairs, guesses);
  if (s) return s;
  return fetch_range(h, first_slot, npairs, results, scores, stats);
}

__global__ void fill_unit_z_normals(float4* n, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) n[i] = make_float4(0.f, 0.f, 1.f, 0.f);
}

// The post-hoc score of IcpUsingPointMatcher::Align (icp_pointmatcher.cc:112-143): ONE FindClosests + TrimmedDist pass of
// the slot's source moved by T against the slot's target; score = exp(-mean distance over the kept matches).  That is
// exactly what a one-iteration IcpFast pass reports (its score comes from the matches made before the pose update), so
// the pass runs through the same kernels; normals play no part in it (a target without normals gets unit-z placeholders).
smhip_status smhip_icp_trimmed_score(smhip_handle h, int slot, const double T[16], float dist_outlier_ratio, double* score, int32_t* kept) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!T || !score) return SMHIP_ERR_INVALID_ARGUMENT;
  if (!(dist_outlier_ratio >= 0.f && dist_outlier_ratio <= 1.f)) { h->err = "dist_outlier_ratio must be in [0, 1]"; return SMHIP_ERR_INVALID_ARGUMENT; }
  if (h->ns[slot] <= 0 || h->nt[slot] <= 0) { h->err = "trimmed score before SetInputSource/SetInputTarget"; return SMHIP_ERR_NOT_READY; }
  HIPCHK(h, hipSetDevice(h->device));
  const int had = h->has_normals[slot];
  if (!had) {
    hipLaunchKernelGGL(fill_unit_z_normals, dim3(ceil_div(h->nt[slot], 256)), dim3(256), 0, h->stream,
                       const_cast<float4*>(h->dev.tgt_n) + (size_t)slot * h->dev.nt_cap, h->nt[slot]);
    h->has_normals[slot] = 1;
  }
  const smhip_icp_options saved = h->opts;
  smhip_icp_options o = saved;
  o.max_iteration = 1; o.early_exit = 0; o.dist_outlier_ratio = dist_outlier_ratio;
  h->opts = o;
  sync_options(h);
  const int comp_was = h->inner_comp;
  h->inner_comp = 0;                       // a rigid pass at T, whatever mode the handle's Aligns run in
  double result[16];
  smhip_icp_stats st{};
  s = enqueue_range(h, slot, 1, T);
  if (s == SMHIP_OK) s = fetch_range(h, slot, 1, result, score, &st);
  h->inner_comp = comp_was;
  h->opts = saved;
  sync_options(h);
  h->has_normals[slot] = had;
  if (kept) *kept = st.kept;
  return s;
}

// The same one-iteration pass for the slots [first, first + npairs) with every match exact, for the information unit
// (smhip_icp_information.hip), which then reads the matches, distances and limits the pass left on the device.  Returns what the
// align calls return: the first failing pair's status, with every pair's own in stats[k].status.  The caller's options are put
// back, and the pass teaches the handle nothing about where a batch's searches thin out.
extern "C++" {
namespace smhip_host {
smhip_status trimmed_pass_range(smhip_context* h, int first, int npairs, const double* Ts, float dist_outlier_ratio, smhip_icp_stats* stats) {
  const smhip_icp_options saved = h->opts;
  smhip_icp_options o = saved;
  o.max_iteration = 1; o.early_exit = 0; o.dist_outlier_ratio = dist_outlier_ratio; o.exact_matches = 1;
  h->opts = o;
  sync_options(h);
  const int comp_was = h->inner_comp;
  h->inner_comp = 0;                       // (rigid, as smhip_icp_trimmed_score)
  smhip_status s = enqueue_range(h, first, npairs, Ts);
  if (s == SMHIP_OK) s = fetch_range(h, first, npairs, nullptr, nullptr, stats);
  else for (int p = 0; p < npairs; ++p) stats[p] = smhip_icp_stats{};
  h->inner_comp = comp_was;
  h->opts = saved;
  sync_options(h);
  h->hist_pairs = 0;
  return s;
}
}  // namespace smhip_host
}

smhip_status smhip_set_target_cache(smhip_handle h, int enable) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  h->target_cache = enable ? 1 : 0;
  return SMHIP_OK;
}

smhip_status smhip_icp_set_inner_compensation(smhip_handle h, int enable) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  if (enable && !h->dev.comp3) {           // the step cloud's array, for every slot, here and never inside an Align
    HIPCHK(h, hipSetDevice(h->device));
    const smhip_status s = dev_alloc(h, &h->dev.comp3, (size_t)h->dev.slots * (size_t)h->dev.ns_cap * 3);
    if (s) return s;
  }
  h->inner_comp = enable ? 1 : 0;
  return SMHIP_OK;
}

smhip_status smhip_icp_get_inner_compensation(smhip_handle h, int* enabled) {
  if (!h || !enabled) return SMHIP_ERR_INVALID_ARGUMENT;
  *enabled = h->inner_comp;
  return SMHIP_OK;
}

smhip_status smhip_icp_forget_search_history(smhip_handle h) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));       // (a batch's rows may still be on their way to hist_pinned)
  h->hist_pairs = 0;
  h->auto_split = 2;
  h->nabo_fused_from = 6;
  return SMHIP_OK;
}

smhip_status smhip_icp_single_launch_counts(smhip_handle h, int64_t* launches_used, int64_t* fallbacks) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  if (launches_used) *launches_used = h->one_launches;
  if (fallbacks) *fallbacks = h->one_fallbacks;
  return SMHIP_OK;
}

smhip_status smhip_get_capacity(smhip_handle h, int* pair_slots, int* max_source_points, int* max_target_points) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  if (pair_slots) *pair_slots = h->dev.slots;
  if (max_source_points) *max_source_points = h->dev.ns_cap;
  if (max_target_points) *max_target_points = h->dev.nt_cap;
  return SMHIP_OK;
}

smhip_status smhip_get_cloud_sizes(smhip_handle h, int slot, int* n_source, int* n_target, int* has_normals) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (n_source) *n_source = h->ns[slot];
  if (n_target) *n_target = h->nt[slot];
  if (has_normals) *has_normals = h->has_normals[slot];
  return SMHIP_OK;
}

smhip_status smhip_icp_align_batch(smhip_handle h, int npairs, const double* guesses, double* results, double* scores,
                                   smhip_icp_stats* stats) {
  smhip_status s = smhip_icp_enqueue_batch(h, npairs, guesses);
  if (s) return s;
  return smhip_icp_fetch_batch(h, npairs, results, scores, stats);
}

smhip_status smhip_icp_align(smhip_handle h, const double guess[16], double result[16], double* score, smhip_icp_stats* stats) {
  return smhip_icp_align_batch(h, 1, guess, result, score, stats);
}

__global__ void export_results(IcpDev b, int npairs, double* out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npairs) return;
  const PairState* st = &b.state[p];
  for (int k = 0; k < 16; ++k) out[18 * p + k] = st->result[k];
  out[18 * p + 16] = st->score;
  // The row has no status column, and its reader (the sequence driver) takes iterations >= 1 for "this pair finished".  A pair that
  // failed after its first iteration keeps the count it reached (finalize's no-correspondence branch and icp_one's bail leave
  // `iter` alone), so a pair that smhip_icp_fetch_batch would answer with a status other than OK exports 0 iterations.
  const bool ok = st->done && st->status == 0 && !st->score_mismatch;
  out[18 * p + 17] = ok ? (double)st->iter : 0.0;
}

smhip_status smhip_icp_export_results_device(smhip_handle h, int npairs, void* dev_out) {
  if (!h || !dev_out || npairs < 1 || npairs > h->dev.slots) return SMHIP_ERR_INVALID_ARGUMENT;
  HIPCHK(h, hipSetDevice(h->device));
  hipLaunchKernelGGL(export_results, dim3(ceil_div(npairs, 64)), dim3(64), 0, h->stream, h->dev, npairs,
                     reinterpret_cast<double*>(dev_out));
  HIPCHK(h, hipGetLastError());
  return SMHIP_OK;
}

smhip_status smhip_icp_get_matches(smhip_handle h, int slot, int32_t* ids, float* d2, int n) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  HIPCHK(h, hipSetDevice(h->device));
  return fetch_matches(h, slot, ids, d2, n);
}

smhip_status smhip_icp_debug_get_grid(smhip_handle h, int slot, double mu[3], float cell_origin[4], int32_t dims[7],
                                      uint32_t* words, int words_cap, uint32_t* cstart, int cstart_cap, float* tq, float* tn, int points_cap) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!mu || !cell_origin || !dims) return SMHIP_ERR_INVALID_ARGUMENT;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->grid_mode[slot] != SMHIP_NN_GRID) { h->err = "debug_get_grid: no search grid is resident in the slot"; return SMHIP_ERR_NOT_READY; }
  PairState st;
  HIPCHK(h, hipMemcpy(&st, h->dev.state + slot, sizeof(PairState), hipMemcpyDeviceToHost));
  for (int d = 0; d < 3; ++d) { mu[d] = st.mu[d]; cell_origin[1 + d] = st.origin[d]; }
  cell_origin[0] = st.h;
  const int32_t geo[7] = {st.nx, st.ny, st.nz, st.wx, st.nw, st.nocc, st.nt};
  for (int k = 0; k < 7; ++k) dims[k] = geo[k];
  if (st.nw < 0 || st.nw > kMaxGridWords || st.nocc < 0 || st.nocc > h->dev.nt_cap || st.nt < 0 || st.nt > h->dev.nt_cap) {
    h->err = "debug_get_grid: the slot's geometry is out of range"; return SMHIP_ERR_NOT_READY;
  }
  const size_t nt_cap = (size_t)h->dev.nt_cap;
  if (words) {
    if (words_cap < st.nw) { h->err = "debug_get_grid: words_cap below nw"; return SMHIP_ERR_CAPACITY; }
    HIPCHK(h, hipMemcpy(words, h->dev.words + (size_t)slot * kMaxGridWords, sizeof(uint2) * (size_t)st.nw, hipMemcpyDeviceToHost));
  }
  if (cstart) {
    if (cstart_cap < st.nocc + 1) { h->err = "debug_get_grid: cstart_cap below nocc + 1"; return SMHIP_ERR_CAPACITY; }
    HIPCHK(h, hipMemcpy(cstart, h->dev.cstart + (size_t)slot * (nt_cap + 1), sizeof(uint32_t) * ((size_t)st.nocc + 1), hipMemcpyDeviceToHost));
  }
  if (tq || tn) {
    if (points_cap < st.nt) { h->err = "debug_get_grid: points_cap below nt"; return SMHIP_ERR_CAPACITY; }
    if (tq) HIPCHK(h, hipMemcpy(tq, h->dev.tq + (size_t)slot * nt_cap, sizeof(float4) * (size_t)st.nt, hipMemcpyDeviceToHost));
    if (tn) HIPCHK(h, hipMemcpy(tn, h->dev.tn + (size_t)slot * nt_cap, sizeof(float4) * (size_t)st.nt, hipMemcpyDeviceToHost));
  }
  return SMHIP_OK;
}

smhip_status smhip_icp_debug_get_kd_tree(smhip_handle h, int slot, double mu[3], float* max_error2, int32_t dims[4],
                                         uint32_t* nodes, int nodes_cap, float* tq, int points_cap, float* leaf, int leaf_cap,
                                         uint8_t* work, float* lb, int queries_cap) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (!h->kd_allocated || h->grid_mode[slot] != SMHIP_NN_NABO) { h->err = "debug_get_kd_tree: no kd-tree is resident in the slot"; return SMHIP_ERR_NOT_READY; }
  PairState st;
  HIPCHK(h, hipMemcpy(&st, h->dev.state + slot, sizeof(PairState), hipMemcpyDeviceToHost));
  if (st.nt < 0 || st.nt > h->dev.nt_cap || st.nocc < 0 || st.nocc > h->kd.node_cap || st.ns < 0 || st.ns > h->dev.ns_cap) {
    h->err = "debug_get_kd_tree: the slot's geometry is out of range"; return SMHIP_ERR_NOT_READY;
  }
  const int blocks = st.nocc > 0 ? (st.nt >> 2) + 1 : 0;        // block index = bucket start >> 2
  if (mu) for (int d = 0; d < 3; ++d) mu[d] = st.mu[d];
  if (max_error2) *max_error2 = kd_max_error2(h);
  if (dims) { dims[0] = st.nocc; dims[1] = st.nt; dims[2] = blocks; dims[3] = st.ns; }
  const size_t nt_cap = (size_t)h->dev.nt_cap, ns_cap = (size_t)h->dev.ns_cap;
  if (nodes) {
    if (nodes_cap < st.nocc) { h->err = "debug_get_kd_tree: nodes_cap below the node count"; return SMHIP_ERR_CAPACITY; }
    HIPCHK(h, hipMemcpy(nodes, h->kd.nodes + (size_t)slot * h->kd.node_cap, sizeof(uint2) * (size_t)st.nocc, hipMemcpyDeviceToHost));
  }
  if (tq) {
    if (points_cap < st.nt) { h->err = "debug_get_kd_tree: points_cap below nt"; return SMHIP_ERR_CAPACITY; }
    HIPCHK(h, hipMemcpy(tq, h->dev.tq + (size_t)slot * nt_cap, sizeof(float4) * (size_t)st.nt, hipMemcpyDeviceToHost));
  }
  if (leaf) {
    if (leaf_cap < blocks || blocks > h->kd.leaf_cap) { h->err = "debug_get_kd_tree: leaf_cap below the block count"; return SMHIP_ERR_CAPACITY; }
    HIPCHK(h, hipMemcpy(leaf, h->kd.leaf + (size_t)slot * h->kd.leaf_cap * 24, sizeof(float) * 24 * (size_t)blocks, hipMemcpyDeviceToHost));
  }
  if (work || lb) {
    if (queries_cap < st.ns) { h->err = "debug_get_kd_tree: queries_cap below ns"; return SMHIP_ERR_CAPACITY; }
    // the device holds the source in its own order: row i came from caller index src.w
    std::vector<float4> src((size_t)st.ns);
    std::vector<uint8_t> w((size_t)st.ns);
    std::vector<float> l((size_t)st.ns);
    HIPCHK(h, hipMemcpy(src.data(), h->dev.src + (size_t)slot * ns_cap, sizeof(float4) * (size_t)st.ns, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(w.data(), h->dev.nabo_work + (size_t)slot * ns_cap, (size_t)st.ns, hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(l.data(), h->dev.lb + (size_t)slot * ns_cap, sizeof(float) * (size_t)st.ns, hipMemcpyDeviceToHost));
    for (int i = 0; i < st.ns; ++i) {
      int32_t orig;
      std::memcpy(&orig, &src[(size_t)i].w, sizeof(orig));
      if (orig < 0 || orig >= st.ns) { h->err = "debug_get_kd_tree: a source row carries no caller index"; return SMHIP_ERR_NOT_READY; }
      if (work) work[orig] = w[(size_t)i];
      if (lb) lb[orig] = l[(size_t)i];
    }
  }
  return SMHIP_OK;
}

smhip_status smhip_icp_find_closests(smhip_handle h, int slot, const double T[16], int32_t* ids, float* d2, int n) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!T) return SMHIP_ERR_INVALID_ARGUMENT;
  if (slot != 0) { h->err = "find_closests works on slot 0"; return SMHIP_ERR_INVALID_ARGUMENT; }
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int ns_max = 0, nt_max = 0;
  // normals are irrelevant for the NN pass
  const int had = h->has_normals[0];
  h->has_normals[0] = 1;
  s = fill_inputs(h, 1, T, &ns_max, &nt_max);
  h->has_normals[0] = had;
  if (s) return s;
  s = enqueue_prepare(h, 1, nt_max);
  if (s) return s;
  const int exact_was = h->dev.exact_all;
  h->dev.exact_all = 1;                 // FindClosests contract: every match exact
  s = enqueue_find_closests(h, 1, ns_max);
  h->dev.exact_all = exact_was;
  if (s) return s;
  s = fetch_matches(h, 0, ids, d2, n);
  // leave the per-iteration scratch clean
  HIPCHK(h, hipMemsetAsync(h->dev.hist, 0, sizeof(uint32_t) * kHistBins, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->ev_used = 0;
  return s;
}

smhip_status smhip_icp_enable_profile(smhip_handle h, int enable) {
  if (!h) return SMHIP_ERR_INVALID_ARGUMENT;
  h->profile = (enable >= 2 && enable <= 4) ? enable : (enable != 0 ? 1 : 0);
  h->prof = smhip_icp_profile{};
  h->ev_used = 0;
  return SMHIP_OK;
}

smhip_status smhip_icp_get_search_counts(smhip_handle h, int slot, uint32_t* counts) {
  smhip_status s = check_slot(h, slot);
  if (s) return s;
  if (!counts) return SMHIP_ERR_INVALID_ARGUMENT;
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(counts, h->dev.search_hist + (size_t)slot * kSearchHist, sizeof(uint32_t) * kSearchHist, hipMemcpyDeviceToHost));
  return SMHIP_OK;
}

smhip_status smhip_icp_get_profile(smhip_handle h, smhip_icp_profile* out) {
  if (!h || !out) return SMHIP_ERR_INVALID_ARGUMENT;
  *out = h->prof;
  return SMHIP_OK;
}

}  // extern "C"
