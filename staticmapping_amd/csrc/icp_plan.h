// icp_plan.h -- which launches an IcpFast call consists of, decided on the host alone.
//
// Pure functions over plain structs: no HIP runtime call, no smhip_context.  smhip_api.hip gathers the settings a decision reads
// into `Inputs` (plan_inputs), asks for the plan and launches what it names; tests/cpp/test_icp_plan.cc asks the same functions
// without a device.  Every threshold of the dispatch is written once, here, with the measurement that justifies it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "smhip_device.h"
#include "../../include/smhip.h"

namespace smhip {
namespace plan {

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
inline int round_up(int a, int b) { return ceil_div(a, b) * b; }

// a batch is split into up to kMaxParts parts on separate streams so that the latency-bound kernels of one part
// (finalize, validate, grid build) hide behind the NN / accumulate kernels of the others
constexpr int kMaxParts = 4;
constexpr int kMinPartPairs = 16;        // pairs a part holds at least (and all but the last a multiple of 8: the XCD mapping)
// the two-launch form pays from ~16 pairs per launch on (measured with the many-lanes-per-query listed search: equal for
// one pair, +4 % at 16, +1 % at 32, +6 % at 2 x 32, +9 % at 256 pairs); an explicit split_after option is honoured
// for any size
constexpr int kTwoLaunchMinPairs = 16;
constexpr int kSmallLaunchBlocks = 512;  // launches of fewer than ~2 workgroups per CU take the small-launch kernel variants
constexpr int kLongChunkBlocks = 768;    // long accumulate chunks once they still leave >= 3 workgroups per CU
constexpr int kCoopMaxQueries = 1 << 21; // ring search: fewer queries than this in the whole launch get several lanes each
constexpr int kOneRoundsPerBlock = 12;   // icp_one: at most 12 rounds per workgroup -- the kernel holds up to kOneMaxRounds = 16 --: measured on 120 000-point
                                         // pairs, 6 pairs at 12 rounds 1.52 ms against 1.71 as separate launches, 8 pairs at 15 rounds 1.87 against 1.73
// shapes of kernels whose constants live beside the kernel (icp_kernels.hip, nabo_kernels.hip); smhip_api.hip asserts that they agree
constexpr int kRingCoopLanes = 4;        // kCoopLanes
constexpr int kNaboBucket = 8;           // kKdBucket
constexpr int kNaboShallowLevels = 12;   // 12 stack levels (40 KiB of LDS) cover the target
constexpr int kShadowMaxTarget = 0x7fff; // the 4-byte shadow of (bound, match) holds 15 bits of match

// ---- the grid build ------------------------------------------------------------------------------------------------------
// Which of the two forms builds the search grid of a launch's targets: true = grid_sort_build (grid_sort_build.hip: one in-LDS stable
// sort per pair, a launch behind tgt_reduce), false = the mark / rank / count / cscan / scatter / place kernels over the zeroed bitmap.
// Both make the same bytes; the sorted form exists for the sort_cells = 1 grid without the row bitmap that the ball search of IcpFast
// walks, and holds a target in one workgroup's registers and LDS: at most 1 024 threads x 32 points, the bound of the shadow word's
// 15-bit match as well.  Everything else -- the 500 k - 2 M-point NDT / GICP targets, sort_cells = 0, the ring-search contexts (row
// bitmap), libnabo's tree -- keeps the kernels it had.  enabled: SMHIP_GRID_BUILD (0 = the old kernels for every launch).
constexpr int kSortBuildMaxTarget = 32768;
// pairs a launch needs for the sorted form.  One workgroup builds a pair whatever the launch holds, where grid_rank cuts a single
// pair's words into 16 segments.  NOT MEASURED yet (profiles/README.md): reasoned from the launches -- two instead of eight on a
// stream where a near-empty launch costs ~5 us, the one workgroup's 2 MiB of `words` about 15 us at a CU's store rate --, so one pair
// takes the sorted form too; tools/small_batch_probe.py of both trees is what moves this number.
constexpr int kSortBuildMinPairs = 1;
inline bool sorted_grid_build(int enabled, int nn_mode, int sort_cells, int have_rowbits, int npairs, int nt_max) {
  return enabled && nn_mode == SMHIP_NN_GRID && sort_cells && !have_rowbits && npairs >= kSortBuildMinPairs && nt_max <= kSortBuildMaxTarget;
}

// ---- capacities ----------------------------------------------------------------------------------------------------------
// the strides smhip_create derives from max_source_points
struct Capacities {
  bool ok;              // finalize indexes at most kFinalizeMaxSeg accumulate waves per pair: 4 Mi source points per cloud
  int acc_blocks, part_stride, dl_stride, bl_stride, seg_stride;
};

inline int certify_blocks(int ns) { return ceil_div(ns, kNnThreads * kCertifyItems); }   // workgroups per pair of the certificate pass
// record segments (one per wave) of accumulate with short chunks: do they fit finalize's table?  (clouds of up to a million points)
inline bool short_chunks_fit(int ns) { return ceil_div(ns, kAccThreads * kAccItemsSmall) * (kAccThreads / 64) <= kFinalizeMaxSeg; }

inline Capacities plan_capacities(int max_source_points) {
  Capacities c{};
  c.ok = max_source_points >= 1 && max_source_points <= kFinalizeMaxSeg * 64 * kAccItemsBatch;
  if (!c.ok) return c;
  const int nbc = certify_blocks(max_source_points);
  c.acc_blocks = ceil_div(max_source_points, kAccThreads * kAccItemsSmall);
  // rows of partials: accumulate's workgroups, or the fused certificate pass's plus accumulate_listed's (reference-search mode)
  c.part_stride = std::max(c.acc_blocks, nbc + std::max(kNaboAccBlocks, kFusedListedMax / kListedSumChunk));
  c.dl_stride = nbc * (kNnThreads * kCertifyItems);
  c.bl_stride = std::max(round_up(max_source_points, kAccThreads * kAccItemsBatch), c.dl_stride);
  // one segment per producing wave: accumulate with short chunks makes the most; the fused path has its certificate pass's waves
  // plus the listed search's
  c.seg_stride = std::max(c.acc_blocks * (kAccThreads / 64),
                          nbc * (kNnThreads / 64) + std::max(kListedBlocks * (kNnThreads / 64), kListedMaxItems) + 1);
  return c;
}

// ---- inputs --------------------------------------------------------------------------------------------------------------
// the resolved settings every decision below reads (what a caller patches around a call -- exact_all, use_ball -- is patched here)
struct Inputs {
  int nn_mode = SMHIP_NN_GRID;
  int use_ball = 1, lds_table = 1, certify = 1, exact_all = 0;
  int split_after = 2;            // resolved: the option, the history's choice (option 0) or never (option < 0)
  int split_after_option = 0;     // as the caller set it: > 0 explicit, 0 follow the history, < 0 never
  int no_fused_sums = 0, no_single_kernel = 0;
  int no_overlap = 0, overlap_streams = 0;
  int nabo_fused_from = 6, sums_long_for = 3, use_shadow = 1, wave_search = 0;
  int sums_blocks = kSumsBlocks, nabo_listed_blocks = 0;
  int one_enabled = 1, one_blocks_want = 0, one_groups_want = 0, one_idle = 0, one_pairs_max = kOnePairs;
  int one_blocks = 0;             // workgroups of icp_one the device holds at once (0: not available)
  int profiling = 0;
  int part_stride = 0, seg_stride = 0;
  int side_streams = 0;           // side streams the handle has
  // Inner motion compensation (smhip_icp_set_inner_compensation): every iteration of an Align starts with comp_apply, which writes the
  // step cloud the other launches then read under an identity pose chain.  The runner-up certificates and the motion potential
  // assume a rigid step, so the mode takes the certificate-free plan: no nn_certify*, no fused pass, no icp_one (compensated()).
  int compensation = 0;
};

// the inputs an Align is planned with: as given, or -- compensation -- with everything that leans on a rigid step switched off
inline Inputs compensated(const Inputs& in) {
  Inputs c = in;
  if (c.compensation) { c.certify = 0; c.no_fused_sums = 1; c.no_single_kernel = 1; }
  return c;
}

// ---- the batch -----------------------------------------------------------------------------------------------------------
struct Part {
  int first = 0, np = 0;    // pairs [first, first + np) of the call
  int nt_max = 0;           // the largest target among them (plan_batch: of the call; the executor narrows it to the part)
  bool small = false;       // few workgroups per launch: the single-round NN / short-chunk accumulate variants
  int acc_items = kAccItemsSmall;
};

struct Batch {
  int nparts = 1;
  Part part[kMaxParts];
  bool one_launch = false;  // the whole loop as the cooperative icp_one, grid (one_grid, npairs)
  int one_grid = 0, one_groups = 8;
  int split_after_used = 0; // smhip_icp_profile::split_after_used
  bool record_history = false;   // copy search_hist back for split_from_history
};

// parts the caller's options ask for (default two.  Measured on 512-pair batches with the fixed-grid tail kernels of round 5: 2 / 3 / 4
// parts = 25.3 / 25.9 / 26.0 k alignments/s, identity guesses 15.3 / 15.8 / 15.7 k, mixed 17.4 / 18.1 / 18.4 k -- overlap_streams = 4 is
// worth 1.5-5 % there; the sequence driver's 256-pair batches lose 12 % with four parts of 64 pairs, so the default stays where every
// batch size is served); 1 when the batch is too small for two
inline int parts_wanted(const Inputs& in, int npairs) {
  const int want = std::min(in.no_overlap ? 1 : (in.overlap_streams > 0 ? in.overlap_streams : 2), kMaxParts);
  return npairs >= 2 * kMinPartPairs ? want : 1;
}

// a part as every launch sizes itself by it
inline Part make_part(int first, int np, int ns_max, int nt_max) {
  Part p;
  p.first = first; p.np = np; p.nt_max = nt_max;
  p.small = np * ceil_div(ns_max, kNnThreads * kBallItems) < kSmallLaunchBlocks;
  // (long chunks also when short ones would make more segments than finalize indexes)
  p.acc_items = (np * ceil_div(ns_max, kAccThreads * kAccItemsBatch) >= kLongChunkBlocks || !short_chunks_fit(ns_max)) ? kAccItemsBatch : kAccItemsSmall;
  return p;
}

// the part of a search outside an Align (find_closests, the GICP correspondences): one launch over every pair, no small variants
inline Part whole_part(int np, int nt_max) {
  Part p;
  p.np = np; p.nt_max = nt_max;
  return p;
}

// is the batch one whose iterations may take the two-launch certificate form without being told to?
inline bool two_launch_sized(int np) { return np >= kTwoLaunchMinPairs; }

inline Batch plan_batch(const Inputs& given, int npairs, int ns_max, int nt_max) {
  const Inputs in = compensated(given);
  Batch b;
  int want = std::min(parts_wanted(in, npairs), 1 + in.side_streams);
  while (want > 1 && npairs < kMinPartPairs * want) --want;
  b.nparts = want;
  for (int k = 0, done = 0; k < want; ++k) {
    int np = (k == want - 1) ? npairs - done : round_up((npairs - done) / (want - k), 8);
    np = std::min(np, npairs - done);
    b.part[k] = make_part(done, np, ns_max, nt_max);
    done += np;
  }
  b.split_after_used = two_launch_sized(npairs) && in.certify ? in.split_after : 0;
  // (only batches that ran the ball search with certificates say anything about where its two forms cross)
  b.record_history = two_launch_sized(npairs) && in.certify &&
                     ((in.split_after_option == 0 && in.nn_mode == SMHIP_NN_GRID && in.use_ball && in.lds_table) || in.nn_mode == SMHIP_NN_NABO);
  // One pair (the front end's call): the whole loop and the score as ONE cooperative launch whose workgroups meet at grid barriers
  // (icp_one.hip) -- the same matches, distances and kept sets as the separate launches.
  // (up to kOnePairs pairs per launch, a row of the grid each: the back end's handful of concurrent submap pairs -- 6 pairs 1.40 ms
  // against 1.71 as separate launches; SMHIP_ONE_PAIRS=n lowers the limit, 1 = single pairs only)
  if (npairs <= std::min(in.one_pairs_max, kOnePairs) && in.one_blocks > 0 && !in.no_single_kernel && in.one_enabled && in.nn_mode == SMHIP_NN_GRID &&
      in.use_ball && in.lds_table && in.certify && !in.exact_all && !in.profiling) {
    const int nrounds = ceil_div(ns_max, kNnThreads);
    // two rounds of 256 points per workgroup (measured on 120 000 points, 20 iterations, target kept: 472 workgroups of one round
    // 1.15-1.18 ms, 320: 1.11-1.15, 240: 1.06-1.11, 160: 1.04-1.13 -- a barrier waits for the slowest workgroup, and two rounds
    // even out what one round's few searching queries cost); a multiple of 8: the barrier's groups.  Several pairs (up to
    // kOnePairs: the back end's handful of concurrent submap pairs) share what the device holds at once, a row of the grid each.
    int G = in.one_blocks_want > 0 ? std::max(8, (in.one_blocks_want / 8) * 8) : round_up(ceil_div(nrounds, 2), 8);
    if (!(in.one_blocks_want > 0 && in.one_idle)) G = std::min(G, round_up(nrounds, 8));   // (SMHIP_ONE_IDLE: tests run small clouds on a grid of mostly idle workgroups)
    if (G >= 64) G = round_up(G, 32);                      // (whole groups of the barrier; workgroups beyond the rounds only take part in the barriers)
    G = std::min(G, ((in.one_blocks / npairs) / 8) * 8);
    if (G >= 8 && ceil_div(nrounds, G) <= std::min(kOneRoundsPerBlock, kOneMaxRounds)) {
      b.one_launch = true;
      b.one_grid = G;
      // the barrier's groups: 8 (measured on 256 / 480 workgroups: 8 or 16 groups equal, 32 groups 7 % slower -- the barriers wait for
      // the slowest workgroup, not for their own atomics; SMHIP_ONE_GROUPS overrides)
      const int w = in.one_groups_want;
      b.one_groups = (w > 0 && (w & (w - 1)) == 0 && w <= 32 && G % w == 0) ? w : 8;
    }
  }
  return b;
}

// ---- one iteration of one part -------------------------------------------------------------------------------------------
enum class Kernel : uint8_t {
  // the ball search, certificate + search in one launch (LDS row tables) or without certificates (nn_ball)
  BallLdsOne, BallLdsFirst, BallLds, BallWaveFirst, BallWave, Ball,
  // the certificate pass alone / with the sums below the predicted band (fused) / the latter on the 4-byte shadow
  CertifyOne, Certify, CertifyAcc, CertifyAccShadow,
  // the search over the queries whose certificate failed: strided over the list, or cut into equal items first
  BallListed, ListedPlan, BallListedItems,
  // refinement of the ball search's bounds
  RefineOne, Validate, RingRefine, Fallback,
  // ring search over every query, brute force
  RingCoop, RingWide, Ring, Brute,
  // libnabo's tree: certificate passes, the walk of the listed queries, the full walk (1 / 4 rounds per workgroup; 12 / kKdStack levels)
  NaboCertifyOne, NaboCertify, NaboCertifyAcc, NaboListedShallow, NaboListedDeep,
  NaboOneShallow, NaboOneDeep, NaboFourShallow, NaboFourDeep, NaboValidate, AccumulateListed,
  // sums and solve
  AccumulateSmall, AccumulateBatch, IterationSumsSmall, IterationSumsBatch, Finalize,
  // inner motion compensation: the step cloud, then the factor-weighted sums and the solve over them (behind the others: their values stay)
  CompApply, AccumulateCompSmall, AccumulateCompBatch, FinalizeComp,
};

// profiling brackets: category 0 prepare, 1 the refinement launches of FindClosests (validate / ring / fallback), 2 error_elements,
// 3 solve, 4 the main NN kernel (fused search, or the full libnabo walk), 5 the certificate pass, 6 the listed search / list walk
enum Category : int8_t { kCatPrepare = 0, kCatRefine = 1, kCatSums = 2, kCatSolve = 3, kCatSearch = 4, kCatCertify = 5, kCatListed = 6 };

struct Launch {
  Kernel kernel;
  int8_t cat;           // profiling category
  bool same_bracket;    // timed together with the launch before it
  int gx, gy;           // grid (gy = 1: an XCD-mapped or fixed 1-D grid)
  int nb;               // XCD-mapped kernels: workgroups per pair (their last argument)
};

struct Iteration {
  int n = 0;
  Launch launch[10];
  // what the kernels of this iteration and part read from IcpDev
  int fused = 0, fused_nabo = 0, acc_items = kAccItemsSmall, sums_items = 0;
  int first_fused = -1;     // the first iteration of this Align that ran the fused path (carried from call to call)

  void add(Kernel k, int cat, int gx, int gy = 1, int nb = 0, bool same_bracket = false) { launch[n++] = Launch{k, (int8_t)cat, same_bracket, gx, gy, nb}; }
  // nb workgroups per pair, consecutive ids dealt round-robin to the 8 XCDs: nb * 8 * ceil(np / 8) workgroups
  void add_xcd(Kernel k, int cat, int nb, int np) { add(k, cat, nb * 8 * ceil_div(np, 8), 1, nb); }
  bool has(Kernel k) const { for (int i = 0; i < n; ++i) if (launch[i].kernel == k) return true; return false; }
  const Launch* find(Kernel k) const { for (int i = 0; i < n; ++i) if (launch[i].kernel == k) return &launch[i]; return nullptr; }
};

// does this iteration of a ball-search part run the certificate pass and the search of the failing queries as two launches?
inline bool two_launch_now(const Inputs& in, const Part& p, int iteration) {
  return in.certify && iteration >= in.split_after && (in.split_after_option > 0 || two_launch_sized(p.np));
}

// Does iteration `iteration` of this batch part run the fused path (nn_certify_acc + nn_ball_listed_items: certificate pass and
// normal-equation sums in one pass over the source)?  Exactly where the two-launch certificate form runs in a batch, unless every
// bound is refined in every iteration anyway (nothing to speculate on) or the cloud has more record segments than finalize indexes.
inline bool fused_now(const Inputs& in, const Part& p, int ns_max, int iteration) {
  if (!in.certify || in.no_fused_sums || p.small) return false;
  const int nbc = certify_blocks(ns_max), seg_cap = std::min(kFinalizeMaxSeg, in.seg_stride);
  if (in.nn_mode == SMHIP_NN_NABO) {
    // the reference-search form: every certificate iteration of a batch (the walk has no bounds to refine); rows of partials for
    // the certificate pass's workgroups + accumulate_listed's
    // ... from the iteration on in which the previous batch's median pair walked fewer than a fifth of its queries again: the walked
    // queries are summed from their lists (accumulate_listed: scattered reads, ten times a streamed point's bytes), which only
    // pays once they are few; before that `accumulate` streams every point
    if (iteration < std::max(1, in.nabo_fused_from) || !two_launch_sized(p.np)) return false;
    return nbc + kNaboAccBlocks <= in.part_stride && nbc * (kNnThreads / 64) + kNaboAccBlocks * (kAccThreads / 64) <= seg_cap;
  }
  if (in.nn_mode != SMHIP_NN_GRID || !in.use_ball || !in.lds_table || in.exact_all) return false;
  if (iteration < 1 || !two_launch_now(in, p, iteration) || p.np > kListedMaxPairs) return false;
  // finalize's segment table: the certificate pass's waves + the listed search's items of a list nn_validate accepts
  return nbc * (kNnThreads / 64) + kListedMaxItems <= seg_cap;
}

// FindClosests of one part: appended to `it`, which carries the iteration's `fused`.  The searches outside an Align (find_closests,
// the GICP correspondences) are iteration 0 of a whole_part.
inline void plan_search(const Inputs& in, const Part& p, int ns_max, int iteration, Iteration& it) {
  const int np = p.np;
  const int nb1 = ceil_div(ns_max, kNnThreads), nbc = certify_blocks(ns_max);
  if (in.nn_mode == SMHIP_NN_NABO) {
    // knn(k = 1, epsilon) through libnabo's tree: what it returns IS the match (no bounds, nothing to refine).  Iteration 0
    // walks every query and records its traversal certificate; later iterations re-walk only the queries that have moved
    // further than their certificate allows (nabo_kernels.hip)
    const bool shallow = p.nt_max <= (kNaboBucket << kNaboShallowLevels);
    if (in.certify && iteration > 0) {
      if (p.small) it.add_xcd(Kernel::NaboCertifyOne, kCatCertify, nb1, np);
      else it.add_xcd(it.fused ? Kernel::NaboCertifyAcc : Kernel::NaboCertify, kCatCertify, nbc, np);   // fused: + the sums below the predicted quantile band
      it.add_xcd(shallow ? Kernel::NaboListedShallow : Kernel::NaboListedDeep, kCatListed, p.small ? nb1 : in.nabo_listed_blocks, np);
      if (it.fused) {
        // the walked queries by the fused pass's rule, and the check of its prediction (this mode's nn_validate)
        it.add(Kernel::NaboValidate, kCatRefine, np);
        it.add(Kernel::AccumulateListed, kCatRefine, kNaboAccBlocks, np, 0, true);
      }
    } else if (p.small) {
      it.add_xcd(shallow ? Kernel::NaboOneShallow : Kernel::NaboOneDeep, kCatSearch, nb1, np);
    } else {
      it.add_xcd(shallow ? Kernel::NaboFourShallow : Kernel::NaboFourDeep, kCatSearch, ceil_div(ns_max, kNnThreads * 4), np);
    }
    return;
  }
  if (in.nn_mode != SMHIP_NN_GRID) {
    it.add(Kernel::Brute, kCatSearch, nb1, np);
    return;
  }
  if (in.use_ball) {
    const int nblk = ceil_div(ns_max, kNnThreads * kBallItems);
    if (in.lds_table && !two_launch_now(in, p, iteration)) {
      // certificate, in-workgroup compaction of the failing queries and LDS-staged search in one launch
      if (p.small) it.add_xcd(Kernel::BallLdsOne, kCatSearch, nb1, np);
      // a wave per 64 queries walks the box of its balls once, candidates broadcast from the wave's LDS strip (nn_ball_wave)
      else if (in.wave_search) it.add_xcd(iteration == 0 ? Kernel::BallWaveFirst : Kernel::BallWave, kCatSearch, nblk, np);
      else it.add_xcd(iteration == 0 ? Kernel::BallLdsFirst : Kernel::BallLds, kCatSearch, nblk, np);
    } else if (in.certify && iteration > 0) {
      // global-memory variant: certificate pass, then a search over the compacted failing queries
      // (also what the converged iterations of the LDS variant use: a streaming certificate pass at full occupancy and a
      // near-empty listed search beat the fused kernel once only a handful of certificates fail)
      const int cat = in.lds_table ? kCatCertify : kCatSearch;
      if (it.fused) {
        // certificate pass + the sums below the predicted quantile band in one pass over the source
        // (every target of the launch below 32 767 points: the 4-byte shadow of bound + match instead of the two arrays.  Only behind
        // the LDS-table ball search, whose kernels -- with the listed search and the refinement kernels -- write the shadow with every
        // match (st_match); nn_ring_wide, nn_brute and nn_nabo set idx / lb alone and never run in such an Align)
        const bool shadow = in.use_shadow && in.lds_table && p.nt_max < kShadowMaxTarget;
        it.add_xcd(shadow ? Kernel::CertifyAccShadow : Kernel::CertifyAcc, cat, nbc, np);
        // the lists' lengths differ by an order of magnitude between the pairs of a launch: cut into equal items first
        it.add(Kernel::ListedPlan, kCatListed, np);
        it.add(Kernel::BallListedItems, kCatListed, kListedItemBlocks, 1, 0, true);
      } else {
        if (p.small) it.add_xcd(Kernel::CertifyOne, cat, nb1, np);
        else it.add_xcd(Kernel::Certify, cat, nbc, np);
        it.add_xcd(Kernel::BallListed, kCatListed, kListedBlocks, np);
      }
    } else {
      it.add_xcd(Kernel::Ball, kCatSearch, nblk, np);
    }
    if ((p.small || it.fused) && !in.exact_all) {
      // a few pairs: validate + ring + fallback as ONE launch, a workgroup per pair (near-empty launches cost ~5 us each there).
      // The same in a batch's fused iterations: the pose has settled there, a quantile that reaches a lower bound is the rare
      // case, and the two spread-out launches cost 20-25 us each of a ~700 us iteration whether they do anything or not
      // (8 192 and 16 384 workgroups that look at one flag).
      it.add(Kernel::RefineOne, kCatRefine, np);
      return;
    }
    it.add(Kernel::Validate, kCatRefine, np);
    it.add(Kernel::RingRefine, kCatRefine, 32, np);
  } else if ((long long)np * ns_max < kCoopMaxQueries) {
    // few queries in the whole launch: several lanes per query keep the SIMDs busy
    it.add(Kernel::RingCoop, kCatSearch, ceil_div(ns_max, kNnThreads / kRingCoopLanes), np);
    it.add(Kernel::RingWide, kCatSearch, kWideBlocks, np, 0, true);
  } else {
    it.add(Kernel::Ring, kCatSearch, nb1, np);
  }
  it.add(Kernel::Fallback, kCatRefine, kFallbackSlices, np);
}

// a search outside an Align
inline Iteration plan_search_only(const Inputs& in, const Part& p, int ns_max) {
  Iteration it;
  plan_search(in, p, ns_max, 0, it);
  return it;
}

// one iteration of one part of an Align: FindClosests, the sums, finalize
inline Iteration plan_iteration(const Inputs& given, const Part& p, int ns_max, int iteration, int first_fused) {
  const Inputs in = compensated(given);
  Iteration it;
  it.first_fused = first_fused;
  it.acc_items = p.acc_items;
  it.fused = fused_now(in, p, ns_max, iteration) ? 1 : 0;     // every launch of this iteration and part sees the same flag
  it.fused_nabo = it.fused && in.nn_mode == SMHIP_NN_NABO ? 1 : 0;
  const bool fused_ball = it.fused && !it.fused_nabo;
  if (fused_ball) {
    // A band needs two quantiles: the iteration after the first has none, so no pair's sums can come from the fused pass -- the
    // plain accumulate launch for all of them (fused = 0 for the sums only would change what finalize expects: keep the flag,
    // it reads spec_ok = 0).  The next `sums_long_for` fused iterations most predictions still miss (the quantile moves by more
    // than a bin): long blocks; after that short ones (iteration_sums), while their record segments -- four per block -- fit
    // finalize's table.
    if (it.first_fused < 0) it.first_fused = iteration;
    it.sums_items = (p.acc_items == kAccItemsBatch && (iteration - it.first_fused < in.sums_long_for || !short_chunks_fit(ns_max))) ? kAccItemsBatch : kAccItemsSmall;
    if (iteration < 2) it.sums_items = p.acc_items;
  }
  // compensation: the step cloud first, a row of the grid per pair (it reads the pair's T_iter from device state)
  if (in.compensation) it.add(Kernel::CompApply, kCatPrepare, ceil_div(ns_max, 256), p.np);
  plan_search(in, p, ns_max, iteration, it);
  const bool batch_items = p.acc_items == kAccItemsBatch;
  if (fused_ball && iteration >= 2) {
    // fused iteration: only the pairs whose prediction missed need `accumulate`, the others the sums of their listed matches --
    // one fixed grid that takes both kinds of work (iteration_sums) instead of workgroups per pair that look at a flag
    it.add(it.sums_items == kAccItemsBatch ? Kernel::IterationSumsBatch : Kernel::IterationSumsSmall, kCatSums, in.sums_blocks);
  } else if (in.compensation) {
    it.add_xcd(batch_items ? Kernel::AccumulateCompBatch : Kernel::AccumulateCompSmall, kCatSums, ceil_div(ns_max, kAccThreads * p.acc_items), p.np);
  } else {
    it.add_xcd(batch_items ? Kernel::AccumulateBatch : Kernel::AccumulateSmall, kCatSums, ceil_div(ns_max, kAccThreads * p.acc_items), p.np);
  }
  it.add(in.compensation ? Kernel::FinalizeComp : Kernel::Finalize, kCatSolve, p.np);
  return it;
}

// ---- history feedback ----------------------------------------------------------------------------------------------------
// The first iteration k >= 1 of the previous batch in which the median pair searched fewer than `split_share` of its queries: where
// certify + listed search starts to beat the fused kernel (measured: the listed search costs ~1 ms per 64 pairs with every query
// listed, the fused kernel 0.25-0.35 ms whatever the share).  rows: [pairs][kSearchHist] searched queries per iteration; no such
// iteration gives max(1, min(iters, kSearchHist)).
inline int split_from_history(const uint32_t* rows, const int* ns, int pairs, int iters, float split_share) {
  int k = 1;
  std::vector<float> share((size_t)pairs);
  for (; k < std::min(iters, kSearchHist); ++k) {
    for (int p = 0; p < pairs; ++p) share[p] = (float)rows[(size_t)p * kSearchHist + k] / (float)std::max(1, ns[p]);
    std::nth_element(share.begin(), share.begin() + share.size() / 2, share.end());
    if (share[share.size() / 2] < split_share) break;
  }
  return k;
}
constexpr int kAutoSplitMax = 8;        // from there on the two-launch form won on every workload measured
constexpr int kNaboFusedFromMax = 12;
inline int clamp_split(int k, int most) { return std::max(1, std::min(k, most)); }

}  // namespace plan
}  // namespace smhip
