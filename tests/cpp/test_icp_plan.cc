// Host test of staticmapping_amd/csrc/icp_plan.h: the rules of the IcpFast dispatch, asserted over a sweep of settings and
// shapes, plus pinned plans of two workloads.  Built with g++ alone (tests/test_icp_plan_cpp.py); no device, no HIP library.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "icp_plan.h"

using namespace smhip;
using namespace smhip::plan;

namespace {

long g_checks = 0, g_failures = 0;
std::string g_case;

#define CHECK(cond)                                                                                         \
  do {                                                                                                      \
    ++g_checks;                                                                                             \
    if (!(cond)) {                                                                                          \
      if (++g_failures <= 20) std::printf("FAILED %s:%d: %s   [%s]\n", __FILE__, __LINE__, #cond, g_case.c_str()); \
    }                                                                                                       \
  } while (0)

int resolved_split(int option) { return option > 0 ? option : (option < 0 ? 1 << 30 : 2); }   // sync_options with the default history

Inputs inputs_for(int ns_cap) {
  const Capacities c = plan_capacities(ns_cap);
  Inputs in;
  in.nabo_listed_blocks = 96;          // kNaboListedBlocks (nabo_kernels.hip)
  in.part_stride = c.part_stride; in.seg_stride = c.seg_stride;
  in.side_streams = 1;
  in.one_blocks = 1024;
  return in;
}

bool is_certificate(Kernel k) {
  return k == Kernel::CertifyOne || k == Kernel::Certify || k == Kernel::CertifyAcc || k == Kernel::CertifyAccShadow ||
         k == Kernel::NaboCertifyOne || k == Kernel::NaboCertify || k == Kernel::NaboCertifyAcc;
}
bool has_certificate(const Iteration& it) { for (int i = 0; i < it.n; ++i) if (is_certificate(it.launch[i].kernel)) return true; return false; }
bool has_ball_certificate(const Iteration& it) {
  return it.has(Kernel::CertifyOne) || it.has(Kernel::Certify) || it.has(Kernel::CertifyAcc) || it.has(Kernel::CertifyAccShadow);
}

// source points one workgroup of an XCD-mapped kernel covers (0: it strides over a list, nothing to cover)
int points_per_block(Kernel k, const Iteration& it) {
  switch (k) {
    case Kernel::BallLdsOne: case Kernel::CertifyOne: case Kernel::NaboCertifyOne: case Kernel::NaboOneShallow: case Kernel::NaboOneDeep: return kNnThreads;
    case Kernel::BallLdsFirst: case Kernel::BallLds: case Kernel::BallWaveFirst: case Kernel::BallWave: case Kernel::Ball: return kNnThreads * kBallItems;
    case Kernel::Certify: case Kernel::CertifyAcc: case Kernel::CertifyAccShadow: case Kernel::NaboCertify: case Kernel::NaboCertifyAcc: return kNnThreads * kCertifyItems;
    case Kernel::NaboFourShallow: case Kernel::NaboFourDeep: return kNnThreads * 4;
    case Kernel::AccumulateSmall: return kAccThreads * kAccItemsSmall;
    case Kernel::AccumulateBatch: return kAccThreads * kAccItemsBatch;
    default: (void)it; return 0;
  }
}

void check_batch(const Inputs& in, const Batch& b, int npairs, int ns_max) {
  int sum = 0;
  CHECK(b.nparts >= 1 && b.nparts <= kMaxParts && b.nparts <= 1 + in.side_streams);
  for (int k = 0; k < b.nparts; ++k) {
    const Part& p = b.part[k];
    CHECK(p.first == sum && p.np >= 1);
    // all parts but the last: multiples of 8 (the XCD mapping) of at least 16 pairs.  The last takes what is left, which the rounding
    // of the others can bring below 16 (39 pairs: 24 + 15) -- such a part keeps to the one-launch search
    if (k + 1 < b.nparts) CHECK(p.np % 8 == 0 && p.np >= 16);
    CHECK(p.small == (p.np * ceil_div(ns_max, kNnThreads * kBallItems) < 512));
    CHECK(p.acc_items == kAccItemsSmall || p.acc_items == kAccItemsBatch);
    sum += p.np;
  }
  CHECK(sum == npairs && npairs >= 16 * b.nparts - (b.nparts == 1 ? 16 : 0));
  if (in.no_overlap) CHECK(b.nparts == 1);
  if (b.one_launch) {
    const int nrounds = ceil_div(ns_max, kNnThreads);
    CHECK(npairs <= kOnePairs && npairs <= in.one_pairs_max);
    CHECK(in.nn_mode == SMHIP_NN_GRID && in.use_ball && in.lds_table && in.certify && !in.exact_all && !in.profiling);
    CHECK(!in.no_single_kernel && in.one_enabled && in.one_blocks > 0);
    CHECK(b.one_grid >= 8 && b.one_grid % 8 == 0 && b.one_grid * npairs <= in.one_blocks && b.one_grid <= kOneMaxBlocks);
    CHECK(ceil_div(nrounds, b.one_grid) <= 12 && ceil_div(nrounds, b.one_grid) <= kOneMaxRounds);
    CHECK(b.one_groups >= 1 && b.one_groups <= 32 && b.one_grid % b.one_groups == 0);
    CHECK(b.nparts == 1);
  }
  CHECK(b.split_after_used == ((npairs >= 16 && in.certify) ? in.split_after : 0));
}

void check_iteration(const Inputs& in, const Part& p, int ns_max, int iteration, const Iteration& it) {
  const bool grid = in.nn_mode == SMHIP_NN_GRID, nabo = in.nn_mode == SMHIP_NN_NABO, ball = grid && in.use_ball;
  const bool explicit_split = in.split_after_option > 0;
  const int seg_cap = std::min(kFinalizeMaxSeg, in.seg_stride);
  CHECK(it.n >= 2 && it.n <= (int)(sizeof(it.launch) / sizeof(it.launch[0])));
  CHECK(it.launch[it.n - 1].kernel == Kernel::Finalize && it.launch[it.n - 1].gx == p.np && it.launch[it.n - 1].cat == kCatSolve);
  CHECK(!it.launch[0].same_bracket);
  for (int i = 1; i < it.n; ++i) if (it.launch[i].same_bracket) CHECK(it.launch[i].cat == it.launch[i - 1].cat);
  // iteration 0 never runs a certificate pass; with no_certify no iteration does
  if (iteration == 0 || !in.certify) CHECK(!has_certificate(it));
  // the fused path
  CHECK(it.fused == 0 || it.fused == 1);
  CHECK(it.fused_nabo == (it.fused && nabo ? 1 : 0));
  CHECK(it.acc_items == p.acc_items);
  if (it.fused) {
    CHECK(grid || nabo);
    CHECK(in.certify && !p.small && !in.no_fused_sums && (p.np >= 16 || explicit_split));
    if (grid) {
      CHECK(!in.exact_all && in.use_ball && in.lds_table && iteration >= std::max(1, in.split_after) && p.np <= kListedMaxPairs);
      const Launch* c = it.find(Kernel::CertifyAcc) ? it.find(Kernel::CertifyAcc) : it.find(Kernel::CertifyAccShadow);
      CHECK(c != nullptr);
      if (c) CHECK(c->nb * (kNnThreads / 64) + kListedMaxItems <= seg_cap);
      CHECK(it.has(Kernel::ListedPlan) && it.has(Kernel::BallListedItems) && !it.has(Kernel::BallListed));
      CHECK(it.sums_items == kAccItemsSmall || it.sums_items == kAccItemsBatch);
      if (iteration >= 2) CHECK(it.has(it.sums_items == kAccItemsBatch ? Kernel::IterationSumsBatch : Kernel::IterationSumsSmall));
      else CHECK(it.sums_items == p.acc_items);
      if (it.has(Kernel::IterationSumsSmall)) CHECK(short_chunks_fit(ns_max));
      CHECK(it.first_fused >= 1 && it.first_fused <= iteration);
    } else {
      CHECK(p.np >= 16 && iteration >= std::max(1, in.nabo_fused_from));
      const Launch* c = it.find(Kernel::NaboCertifyAcc);
      CHECK(c != nullptr);
      if (c) {
        CHECK(c->nb * (kNnThreads / 64) + kNaboAccBlocks * (kAccThreads / 64) <= seg_cap);
        CHECK(c->nb + kNaboAccBlocks <= in.part_stride);
      }
      CHECK(it.has(Kernel::NaboValidate) && it.has(Kernel::AccumulateListed));
    }
  } else {
    CHECK(it.sums_items == 0);
    CHECK(!it.has(Kernel::CertifyAcc) && !it.has(Kernel::CertifyAccShadow) && !it.has(Kernel::NaboCertifyAcc) && !it.has(Kernel::ListedPlan));
    CHECK(!it.has(Kernel::IterationSumsSmall) && !it.has(Kernel::IterationSumsBatch));
    // ... and runs wherever the two-launch form runs in a batch and its segments fit
    if (ball && in.lds_table && in.certify && !in.exact_all && !in.no_fused_sums && !p.small && iteration >= std::max(1, in.split_after) &&
        (explicit_split || p.np >= 16) && p.np <= kListedMaxPairs)
      CHECK(certify_blocks(ns_max) * (kNnThreads / 64) + kListedMaxItems > seg_cap);
  }
  // whenever accumulate runs, its segments fit finalize's table
  for (Kernel k : {Kernel::AccumulateSmall, Kernel::AccumulateBatch})
    if (const Launch* a = it.find(k)) CHECK(a->nb * (kAccThreads / 64) <= kFinalizeMaxSeg && a->nb <= in.part_stride);
  CHECK((int)it.has(Kernel::AccumulateSmall) + it.has(Kernel::AccumulateBatch) + it.has(Kernel::IterationSumsSmall) + it.has(Kernel::IterationSumsBatch) == 1);
  // the shadow form
  if (it.has(Kernel::CertifyAccShadow)) CHECK(in.lds_table && in.use_shadow && p.nt_max < 0x7fff);
  if (it.has(Kernel::CertifyAcc)) CHECK(!(in.lds_table && in.use_shadow && p.nt_max < 0x7fff));
  // refinement
  const bool refine_one = ball && (p.small || it.fused) && !in.exact_all;
  CHECK(it.has(Kernel::RefineOne) == refine_one);
  if (refine_one) CHECK(!it.has(Kernel::Validate) && !it.has(Kernel::RingRefine) && !it.has(Kernel::Fallback));
  else if (ball) CHECK(it.has(Kernel::Validate) && it.has(Kernel::RingRefine) && it.has(Kernel::Fallback));
  if (grid && !in.use_ball) CHECK(it.has(Kernel::Fallback) && (it.has(Kernel::Ring) != it.has(Kernel::RingCoop)) && it.has(Kernel::RingCoop) == it.has(Kernel::RingWide));
  if (!grid) CHECK(!it.has(Kernel::Fallback) && !it.has(Kernel::Validate) && !it.has(Kernel::RefineOne));
  if (!grid && !nabo) CHECK(it.has(Kernel::Brute) && it.n == 3);
  // the two-launch form of the ball search
  if (ball) {
    const bool two = in.lds_table ? (in.certify && iteration >= in.split_after && (explicit_split || p.np >= 16)) : (in.certify && iteration > 0);
    CHECK(has_ball_certificate(it) == two);
    CHECK((it.has(Kernel::BallListed) || it.has(Kernel::BallListedItems)) == two);
    const bool one = it.has(Kernel::BallLdsOne) || it.has(Kernel::BallLdsFirst) || it.has(Kernel::BallLds) || it.has(Kernel::BallWaveFirst) || it.has(Kernel::BallWave);
    CHECK(one == (in.lds_table && !two));
    CHECK(it.has(Kernel::Ball) == (!in.lds_table && !two));
    if (it.has(Kernel::BallWaveFirst) || it.has(Kernel::BallWave)) CHECK(in.wave_search && !p.small);
    CHECK((it.has(Kernel::BallLdsFirst) || it.has(Kernel::BallWaveFirst)) == (one && !p.small && iteration == 0));
    CHECK(it.has(Kernel::BallLdsOne) == (one && p.small));
  } else {
    CHECK(!has_ball_certificate(it) && !it.has(Kernel::Ball) && !it.has(Kernel::BallLds) && !it.has(Kernel::BallListed));
  }
  if (nabo) {
    const bool shallow = p.nt_max <= (8 << 12);
    CHECK(!(it.has(Kernel::NaboListedDeep) || it.has(Kernel::NaboOneDeep) || it.has(Kernel::NaboFourDeep)) || !shallow);
    CHECK(!(it.has(Kernel::NaboListedShallow) || it.has(Kernel::NaboOneShallow) || it.has(Kernel::NaboFourShallow)) || shallow);
    CHECK(has_certificate(it) == (in.certify && iteration > 0));
  }
  // grids
  for (int i = 0; i < it.n; ++i) {
    const Launch& l = it.launch[i];
    CHECK(l.gx >= 1 && l.gy >= 1 && l.cat >= 0 && l.cat <= 6);
    if (l.nb > 0) {     // XCD-mapped
      CHECK(l.gy == 1 && l.gx % 8 == 0 && l.gx == l.nb * 8 * ceil_div(p.np, 8));
      const int ppb = points_per_block(l.kernel, it);
      if (ppb) CHECK((long long)l.nb * ppb >= ns_max && (long long)(l.nb - 1) * ppb < ns_max);
    } else if (l.gy > 1 || l.kernel == Kernel::Ring || l.kernel == Kernel::RingCoop || l.kernel == Kernel::Brute) {
      CHECK(l.gy == p.np);
    }
    if (l.kernel == Kernel::IterationSumsSmall || l.kernel == Kernel::IterationSumsBatch) CHECK(l.gx == in.sums_blocks && l.gy == 1);
    if (l.kernel == Kernel::Ring || l.kernel == Kernel::Brute) CHECK((long long)l.gx * kNnThreads >= ns_max);
    if (l.kernel == Kernel::RingCoop) CHECK((long long)l.gx * (kNnThreads / 4) >= ns_max && (long long)p.np * ns_max < (1ll << 21));
  }
}

void sweep() {
  const int modes[] = {SMHIP_NN_BRUTE, SMHIP_NN_GRID, SMHIP_NN_NABO};
  const int splits[] = {-1, 0, 1, 5};
  const int pairs[] = {1, 8, 15, 16, 31, 32, 64, 256, 1024, 1025};
  const int sources[] = {256, 20000, 120000, 1100000, 4194304};
  const int targets[] = {5000, 32766, 32767, 500000};
  char buf[256];
  for (int ns_max : sources) {
    CHECK(plan_capacities(ns_max).ok);
    for (int mode : modes) for (int use_ball = 0; use_ball < 2; ++use_ball) for (int no_lds = 0; no_lds < 2; ++no_lds)
    for (int no_certify = 0; no_certify < 2; ++no_certify) for (int exact = 0; exact < 2; ++exact) for (int no_fused = 0; no_fused < 2; ++no_fused)
    for (int split : splits) for (int wave = 0; wave < 2; ++wave) for (int shadow = 0; shadow < 2; ++shadow) {
      Inputs in = inputs_for(ns_max);        // the strides of a handle made for exactly this cloud: the tightest case
      in.nn_mode = mode; in.use_ball = use_ball; in.lds_table = !no_lds; in.certify = !no_certify; in.exact_all = exact;
      in.no_fused_sums = no_fused; in.split_after_option = split; in.split_after = resolved_split(split);
      in.wave_search = wave; in.use_shadow = shadow;
      for (int npairs : pairs) for (int nt_max : targets) {
        std::snprintf(buf, sizeof(buf), "mode %d ball %d lds %d certify %d exact %d no_fused %d split %d wave %d shadow %d npairs %d ns %d nt %d",
                      mode, use_ball, !no_lds, !no_certify, exact, no_fused, split, wave, shadow, npairs, ns_max, nt_max);
        g_case = buf;
        const Batch b = plan_batch(in, npairs, ns_max, nt_max);
        check_batch(in, b, npairs, ns_max);
        for (int k = 0; k < b.nparts; ++k) {
          int first_fused = -1;
          bool was_fused = false;
          for (int iteration = 0; iteration < 10; ++iteration) {
            const Iteration it = plan_iteration(in, b.part[k], ns_max, iteration, first_fused);
            g_case = std::string(buf) + " part " + std::to_string(k) + " iteration " + std::to_string(iteration);
            check_iteration(in, b.part[k], ns_max, iteration, it);
            CHECK(!was_fused || it.fused);      // once fused, an Align stays fused
            if (!it.fused || it.fused_nabo) CHECK(it.first_fused == first_fused);
            else CHECK(it.first_fused == (first_fused < 0 ? iteration : first_fused));
            was_fused = it.fused;
            first_fused = it.first_fused;
          }
        }
        // a search outside an Align: the same FindClosests as iteration 0 of a part that is never small, nothing else
        const Part w = whole_part(npairs, nt_max);
        const Iteration s = plan_search_only(in, w, ns_max);
        const Iteration full = plan_iteration(in, w, ns_max, 0, -1);
        CHECK(s.n == full.n - 2 && s.fused == 0 && !has_certificate(s) && !s.has(Kernel::Finalize));
        for (int i = 0; i < s.n; ++i) CHECK(std::memcmp(&s.launch[i], &full.launch[i], sizeof(Launch)) == 0);
      }
    }
  }
}

void parts_and_one_launch() {
  g_case = "parts";
  for (int overlap = 0; overlap <= 5; ++overlap) for (int no_overlap = 0; no_overlap < 2; ++no_overlap) for (int side = 0; side <= 3; ++side)
    for (int npairs = 1; npairs <= 1100; npairs += (npairs < 140 ? 1 : 37)) {
      Inputs in = inputs_for(120000);
      in.overlap_streams = overlap; in.no_overlap = no_overlap; in.side_streams = side; in.split_after = 2;
      const Batch b = plan_batch(in, npairs, 120000, 30000);
      check_batch(in, b, npairs, 120000);
      const int asked = no_overlap ? 1 : std::min(overlap > 0 ? overlap : 2, kMaxParts);
      CHECK(b.nparts == std::max(1, std::min(std::min(asked, 1 + side), npairs / 16)));
      CHECK(parts_wanted(in, npairs) == (npairs >= 32 ? asked : 1));
    }
  g_case = "one launch";
  for (int ns_max : {1, 256, 2000, 20000, 120000, 130000, 1100000}) for (int npairs = 1; npairs <= 9; ++npairs)
    for (int one_blocks : {0, 256, 512, 1024}) for (int want : {0, 8, 64, 100, 480}) for (int idle = 0; idle < 2; ++idle) for (int pairs_max : {1, 4, 8}) for (int groups : {0, 3, 16, 32, 64}) {
      Inputs in = inputs_for(1100000);
      in.one_blocks = one_blocks; in.one_blocks_want = want; in.one_idle = idle; in.one_pairs_max = pairs_max; in.one_groups_want = groups;
      const Batch b = plan_batch(in, npairs, ns_max, 30000);
      check_batch(in, b, npairs, ns_max);
      if (b.one_launch && !(want > 0 && idle)) CHECK(b.one_grid <= round_up(ceil_div(ns_max, kNnThreads), 32));   // no grid of idle workgroups unless asked for
      if (b.one_launch) CHECK(b.one_groups == ((groups == 16 || groups == 32) && b.one_grid % groups == 0 ? groups : 8));
      for (int off = 0; off < 6; ++off) {      // every setting the launch depends on switches it off
        Inputs o = in;
        switch (off) {
          case 0: o.no_single_kernel = 1; break;
          case 1: o.one_enabled = 0; break;
          case 2: o.profiling = 1; break;
          case 3: o.exact_all = 1; break;
          case 4: o.nn_mode = SMHIP_NN_NABO; break;
          case 5: o.lds_table = 0; break;
        }
        CHECK(!plan_batch(o, npairs, ns_max, 30000).one_launch);
      }
    }
  {   // the front end's call: one pair of 120 000 points, 469 rounds, two per workgroup
    const Batch b = plan_batch(inputs_for(120000), 1, 120000, 30000);
    CHECK(b.one_launch && b.one_grid == 256 && b.one_groups == 8);
  }
}

void history() {
  g_case = "history";
  const int P = 5, ns[P] = {1000, 1000, 1000, 1000, 1000};
  std::vector<uint32_t> rows((size_t)P * kSearchHist);
  auto fill = [&](auto share_of) { for (int p = 0; p < P; ++p) for (int k = 0; k < kSearchHist; ++k) rows[(size_t)p * kSearchHist + k] = (uint32_t)(1000 * share_of(p, k)); };
  fill([](int, int k) { return k < 4 ? 0.9 : 0.1; });                      // every pair drops below a fifth at iteration 4
  CHECK(split_from_history(rows.data(), ns, P, 20, 0.2f) == 4);
  fill([](int p, int k) { return (k >= 3 && p < 3) || k >= 6 ? 0.1 : 0.9; });   // the median pair (three of five) at 3, the others at 6
  CHECK(split_from_history(rows.data(), ns, P, 20, 0.2f) == 3);
  fill([](int p, int k) { return (k >= 3 && p < 2) || k >= 6 ? 0.1 : 0.9; });   // two of five are not the median
  CHECK(split_from_history(rows.data(), ns, P, 20, 0.2f) == 6);
  fill([](int, int k) { return k == 0 ? 0.0 : 0.9; });                     // iteration 0 does not count; no such k
  CHECK(split_from_history(rows.data(), ns, P, 20, 0.2f) == kSearchHist);
  CHECK(split_from_history(rows.data(), ns, P, 5, 0.2f) == 5);
  CHECK(split_from_history(rows.data(), ns, P, 1, 0.2f) == 1);
  CHECK(split_from_history(rows.data(), ns, P, 0, 0.2f) == 1);
  fill([](int, int) { return 0.19; });
  CHECK(split_from_history(rows.data(), ns, P, 20, 0.2f) == 1);
  CHECK(split_from_history(rows.data(), ns, P, 20, 0.19f) == kSearchHist);   // below, not at, the threshold
  const int big[P] = {10000, 10000, 10000, 10000, 10000};                   // shares are of each pair's own source
  CHECK(split_from_history(rows.data(), big, P, 20, 0.05f) == 1);
  CHECK(clamp_split(0, kAutoSplitMax) == 1 && clamp_split(12, kAutoSplitMax) == 8 && clamp_split(12, kNaboFusedFromMax) == 12 && clamp_split(5, kAutoSplitMax) == 5);
}

void capacities() {
  g_case = "capacities";
  CHECK(plan_capacities(4194304).ok && !plan_capacities(4194305).ok && !plan_capacities(0).ok);
  for (int n : {1, 255, 256, 257, 8192, 8193, 120000, 1100000, 4194304}) {
    const Capacities c = plan_capacities(n);
    CHECK(c.acc_blocks == ceil_div(n, 2048) && c.part_stride >= c.acc_blocks && c.part_stride >= ceil_div(n, 8192) + kNaboAccBlocks);
    CHECK(c.dl_stride >= n && c.dl_stride % 8192 == 0 && c.bl_stride >= c.dl_stride && c.bl_stride % 8192 == 0);
    CHECK(c.seg_stride >= c.acc_blocks * 4 && c.seg_stride > ceil_div(n, 8192) * 4 + kListedMaxItems && c.seg_stride > ceil_div(n, 8192) * 4 + kListedBlocks * 4);
  }
  const Capacities c = plan_capacities(120000);     // 59 short accumulate blocks, 15 certificate-pass blocks
  CHECK(c.acc_blocks == 59 && c.part_stride == 59 && c.dl_stride == 122880 && c.bl_stride == 122880 && c.seg_stride == 236);
}

struct Row { Kernel k; int gx, gy; };
void expect(const Iteration& it, std::initializer_list<Row> rows) {
  CHECK(it.n == (int)rows.size());
  int i = 0;
  for (const Row& r : rows) {
    if (i < it.n) CHECK(it.launch[i].kernel == r.k && it.launch[i].gx == r.gx && it.launch[i].gy == r.gy);
    ++i;
  }
}

// read off the dispatch as it stood before the plan existed; defaults, split_after resolved to 2, a handle made for 120 000 source points
void pinned() {
  Inputs in = inputs_for(120000);
  {
    g_case = "pinned: part of 256 pairs";
    const Part p = make_part(0, 256, 120000, 30000);
    CHECK(!p.small && p.acc_items == 32);
    int ff = -1;
    for (int iteration = 0; iteration < 2; ++iteration) {
      const Iteration it = plan_iteration(in, p, 120000, iteration, ff);
      expect(it, {{iteration == 0 ? Kernel::BallLdsFirst : Kernel::BallLds, 235 * 8 * 32, 1}, {Kernel::Validate, 256, 1}, {Kernel::RingRefine, 32, 256},
                  {Kernel::Fallback, 64, 256}, {Kernel::AccumulateBatch, 15 * 8 * 32, 1}, {Kernel::Finalize, 256, 1}});
      CHECK(!it.fused && it.first_fused == -1);
      CHECK(it.launch[0].cat == kCatSearch && it.launch[1].cat == kCatRefine && it.launch[4].cat == kCatSums && it.launch[5].cat == kCatSolve);
    }
    for (int iteration = 2; iteration < 8; ++iteration) {
      const Iteration it = plan_iteration(in, p, 120000, iteration, ff);
      ff = it.first_fused;
      expect(it, {{Kernel::CertifyAccShadow, 3840, 1}, {Kernel::ListedPlan, 256, 1}, {Kernel::BallListedItems, 1280, 1}, {Kernel::RefineOne, 256, 1},
                  {iteration < 5 ? Kernel::IterationSumsBatch : Kernel::IterationSumsSmall, 2048, 1}, {Kernel::Finalize, 256, 1}});
      CHECK(it.fused && !it.fused_nabo && ff == 2 && it.sums_items == (iteration < 5 ? 32 : 8) && it.acc_items == 32);
      CHECK(it.launch[0].cat == kCatCertify && it.launch[1].cat == kCatListed && it.launch[2].cat == kCatListed && it.launch[2].same_bracket && it.launch[3].cat == kCatRefine);
    }
  }
  {
    g_case = "pinned: one pair, separate launches";
    in.no_single_kernel = 1;
    const Batch b = plan_batch(in, 1, 120000, 30000);
    CHECK(!b.one_launch && b.nparts == 1 && b.part[0].small && b.part[0].acc_items == 8 && b.split_after_used == 0 && !b.record_history);
    for (int iteration = 0; iteration < 10; ++iteration) {
      const Iteration it = plan_iteration(in, b.part[0], 120000, iteration, -1);
      expect(it, {{Kernel::BallLdsOne, 469 * 8, 1}, {Kernel::RefineOne, 1, 1}, {Kernel::AccumulateSmall, 59 * 8, 1}, {Kernel::Finalize, 1, 1}});
      CHECK(!it.fused);
    }
  }
}

// The launch shapes tests/test_nabo_exact_gpu.py names, as the plan decides them (tests/nabo_cases.py holds the same sizes: 32 slots,
// 7 700 queries, targets of 8 << 12 and 8 << 12 + 1 points): which nn_nabo instantiation walks and how the list walk is laid out.
void nabo_exact_cases() {
  constexpr int NS = 7700, SLOTS = 32;
  for (int nt : {8 << 12, (8 << 12) + 1}) {
    const bool shallow = nt <= 8 << 12;
    Inputs in = inputs_for(NS);
    in.nn_mode = SMHIP_NN_NABO;
    {
      g_case = "nabo exact: find_closests, a search outside an Align -- four rounds per workgroup whatever the size";
      for (int ns : {1, 400, 1025, 4096, 20000}) {
        const Iteration it = plan_search_only(in, whole_part(1, nt), ns);
        expect(it, {{shallow ? Kernel::NaboFourShallow : Kernel::NaboFourDeep, ceil_div(ns, 1024) * 8, 1}});
      }
    }
    {
      g_case = "nabo exact: one pair's Align -- one round per workgroup, the list walk on as many workgroups";
      const Batch b = plan_batch(in, 1, NS, nt);
      CHECK(b.nparts == 1 && b.part[0].small && !b.one_launch);
      const Iteration i0 = plan_iteration(in, b.part[0], NS, 0, -1), i1 = plan_iteration(in, b.part[0], NS, 1, -1);
      CHECK(i0.n == 3 && i0.launch[0].kernel == (shallow ? Kernel::NaboOneShallow : Kernel::NaboOneDeep) && i0.launch[0].nb == 31);
      CHECK(i1.n == 4 && i1.launch[0].kernel == Kernel::NaboCertifyOne && i1.launch[0].nb == 31);
      CHECK(i1.launch[1].kernel == (shallow ? Kernel::NaboListedShallow : Kernel::NaboListedDeep) && i1.launch[1].nb == 31 && !i1.fused);
    }
    {
      g_case = "nabo exact: 32 pairs with the default overlap -- two parts of 16 pairs, 256 workgroups each: the small forms again";
      const Batch b = plan_batch(in, SLOTS, NS, nt);
      CHECK(b.nparts == 2 && b.part[0].np == 16 && b.part[1].np == 16 && b.part[0].small && b.part[1].small);
      const Iteration i0 = plan_iteration(in, b.part[1], NS, 0, -1), i1 = plan_iteration(in, b.part[1], NS, 1, -1);
      CHECK(i0.launch[0].kernel == (shallow ? Kernel::NaboOneShallow : Kernel::NaboOneDeep));
      CHECK(i1.launch[0].kernel == Kernel::NaboCertifyOne && i1.launch[1].nb == 31);
    }
    for (int listed : {96, 8}) {
      g_case = "nabo exact: 32 pairs as one part (no_overlap) -- 512 workgroups: four rounds, the batch certificate pass, the strided list walk";
      in.no_overlap = 1;
      in.nabo_listed_blocks = listed;              // 96: kNaboListedBlocks; 8: SMHIP_NABO_LISTED_BLOCKS=8, 2 048 queries a trip
      const Batch b = plan_batch(in, SLOTS, NS, nt);
      CHECK(b.nparts == 1 && b.part[0].np == SLOTS && !b.part[0].small && SLOTS * ceil_div(NS, 512) == 512);
      const Iteration i0 = plan_iteration(in, b.part[0], NS, 0, -1), i1 = plan_iteration(in, b.part[0], NS, 1, -1);
      CHECK(i0.n == 3 && i0.launch[0].kernel == (shallow ? Kernel::NaboFourShallow : Kernel::NaboFourDeep) && i0.launch[0].nb == 8);
      CHECK(i1.n == 4 && i1.launch[0].kernel == Kernel::NaboCertify && i1.launch[0].nb == certify_blocks(NS) && !i1.fused);
      CHECK(i1.launch[1].kernel == (shallow ? Kernel::NaboListedShallow : Kernel::NaboListedDeep) && i1.launch[1].nb == listed);
      in.no_overlap = 0;
    }
  }
}

}  // namespace

int main() {
  capacities();
  history();
  pinned();
  nabo_exact_cases();
  parts_and_one_launch();
  sweep();
  std::printf("%ld checks, %ld failed\n", g_checks, g_failures);
  if (g_failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
