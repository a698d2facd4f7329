// Host test of the inner-compensation plan (staticmapping_amd/csrc/icp_plan.h, Inputs::compensation), for 1, 4, 16 and 64 pairs:
// no one_launch, no certificate or fused kernel in any iteration, comp_apply first, the rest the rigid certificate-free plan
// kernel for kernel -- and with the flag off the plans are, field by field, the ones the header made before it knew the flag
// (kPinned: a hash taken with that header).  Built with g++ alone (tests/test_icp_plan_comp_cpp.py); no device, no HIP library.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

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

Inputs inputs_for(int ns_cap) {
  const Capacities c = plan_capacities(ns_cap);
  Inputs in;
  in.nabo_listed_blocks = 96;
  in.part_stride = c.part_stride; in.seg_stride = c.seg_stride;
  in.side_streams = 1;
  in.one_blocks = 1024;
  return in;
}

// FNV-1a over the fields that mean something (an Iteration's launches beyond n and the structs' padding are not data)
struct Hash {
  uint64_t h = 1469598103934665603ull;
  void add(long long v) { for (int k = 0; k < 8; ++k) { h ^= (uint64_t)((v >> (8 * k)) & 0xff); h *= 1099511628211ull; } }
};
void hash_batch(Hash& H, const Batch& b) {
  H.add(b.nparts); H.add(b.one_launch); H.add(b.one_grid); H.add(b.one_groups); H.add(b.split_after_used); H.add(b.record_history);
  for (int k = 0; k < b.nparts; ++k) { const Part& p = b.part[k]; H.add(p.first); H.add(p.np); H.add(p.nt_max); H.add(p.small); H.add(p.acc_items); }
}
void hash_iteration(Hash& H, const Iteration& it) {
  H.add(it.n); H.add(it.fused); H.add(it.fused_nabo); H.add(it.acc_items); H.add(it.sums_items); H.add(it.first_fused);
  for (int i = 0; i < it.n; ++i) {
    const Launch& l = it.launch[i];
    H.add((int)l.kernel); H.add(l.cat); H.add(l.same_bracket); H.add(l.gx); H.add(l.gy); H.add(l.nb);
  }
}

#ifndef SMHIP_PLAN_PIN_ONLY
bool forbidden(Kernel k) {     // everything that leans on a rigid step
  switch (k) {
    case Kernel::CertifyOne: case Kernel::Certify: case Kernel::CertifyAcc: case Kernel::CertifyAccShadow:
    case Kernel::NaboCertifyOne: case Kernel::NaboCertify: case Kernel::NaboCertifyAcc:
    case Kernel::BallListed: case Kernel::ListedPlan: case Kernel::BallListedItems:
    case Kernel::IterationSumsSmall: case Kernel::IterationSumsBatch: case Kernel::AccumulateListed: case Kernel::NaboValidate:
      return true;
    default: return false;
  }
}
Kernel rigid_form(Kernel k) {
  switch (k) {
    case Kernel::AccumulateCompSmall: return Kernel::AccumulateSmall;
    case Kernel::AccumulateCompBatch: return Kernel::AccumulateBatch;
    case Kernel::FinalizeComp: return Kernel::Finalize;
    default: return k;
  }
}
#endif

constexpr int kPairs[4] = {1, 4, 16, 64};
constexpr int kIterations = 20;
struct Shape { int ns, nt; };
constexpr Shape kShapes[3] = {{3000, 900}, {20000, 4096}, {120000, 24000}};

// the plans of every setting of the sweep below with the flag off, hashed with the header as it was before Inputs::compensation
// (this file built with -DSMHIP_PLAN_PIN_ONLY against that header, run with --print-pin)
constexpr uint64_t kPinned = 0x165e3d045b2eba99ull;

}  // namespace

int main(int argc, char** argv) {
  Hash pinned;
  for (const Shape& sh : kShapes) {
    for (int np : kPairs) {
      for (int variant = 0; variant < 4; ++variant) {
        Inputs in = inputs_for(sh.ns);
        in.side_streams = 3;
        if (variant == 1) in.use_ball = 0;
        if (variant == 2) in.lds_table = 0;
        if (variant == 3) { in.split_after_option = 3; in.split_after = 3; }
        g_case = "ns " + std::to_string(sh.ns) + " pairs " + std::to_string(np) + " variant " + std::to_string(variant);
        // ---- flag off: today's plans
        const Batch off = plan_batch(in, np, sh.ns, sh.nt);
        hash_batch(pinned, off);
        for (int k = 0; k < off.nparts; ++k) {
          int ff = -1;
          for (int it = 0; it < kIterations; ++it) {
            const Iteration p = plan_iteration(in, off.part[k], sh.ns, it, ff);
            ff = p.first_fused;
            hash_iteration(pinned, p);
#ifndef SMHIP_PLAN_PIN_ONLY
            CHECK(!p.has(Kernel::CompApply) && !p.has(Kernel::FinalizeComp) && !p.has(Kernel::AccumulateCompSmall) && !p.has(Kernel::AccumulateCompBatch));
#endif
          }
        }
#ifndef SMHIP_PLAN_PIN_ONLY
        // ---- flag on
        Inputs on = in;
        on.compensation = 1;
        Inputs rigid = in;                       // the rigid form of the same plan
        rigid.certify = 0; rigid.no_single_kernel = 1; rigid.no_fused_sums = 1;
        const Batch b = plan_batch(on, np, sh.ns, sh.nt), r = plan_batch(rigid, np, sh.ns, sh.nt);
        CHECK(!b.one_launch);
        CHECK(b.split_after_used == 0 && !b.record_history);
        {
          Hash hb, hr;
          hash_batch(hb, b); hash_batch(hr, r);
          CHECK(hb.h == hr.h);
        }
        if (np == 1 && variant == 0) CHECK(off.one_launch);       // (what the flag switches off is there without it)
        for (int k = 0; k < b.nparts; ++k) {
          int ff = -1, ffr = -1;
          for (int it = 0; it < kIterations; ++it) {
            const Iteration p = plan_iteration(on, b.part[k], sh.ns, it, ff), q = plan_iteration(rigid, r.part[k], sh.ns, it, ffr);
            ff = p.first_fused; ffr = q.first_fused;
            CHECK(p.n >= 4 && p.n <= 10);
            CHECK(p.launch[0].kernel == Kernel::CompApply);
            CHECK(p.launch[0].gx == ceil_div(sh.ns, 256) && p.launch[0].gy == b.part[k].np);      // a row of the grid per pair, every source row covered
            CHECK(p.fused == 0 && p.fused_nabo == 0 && p.first_fused == -1);
            for (int i = 0; i < p.n; ++i) CHECK(!forbidden(p.launch[i].kernel));
            for (int i = 1; i < p.n; ++i) CHECK(p.launch[i].kernel != Kernel::CompApply);
            CHECK(p.launch[p.n - 1].kernel == Kernel::FinalizeComp);
            CHECK(p.has(Kernel::AccumulateCompSmall) || p.has(Kernel::AccumulateCompBatch));
            CHECK(!p.has(Kernel::AccumulateSmall) && !p.has(Kernel::AccumulateBatch) && !p.has(Kernel::Finalize));
            // behind comp_apply: the rigid certificate-free iteration, launch for launch
            CHECK(p.n == q.n + 1);
            for (int i = 0; i + 1 < p.n && i < q.n; ++i) {
              const Launch &a = p.launch[i + 1], &c = q.launch[i];
              CHECK(rigid_form(a.kernel) == c.kernel && a.cat == c.cat && a.same_bracket == c.same_bracket && a.gx == c.gx && a.gy == c.gy && a.nb == c.nb);
            }
          }
        }
#endif
      }
    }
  }
  if (argc > 1 && std::strcmp(argv[1], "--print-pin") == 0) { std::printf("0x%016llxull\n", (unsigned long long)pinned.h); return 0; }
  g_case = "pinned plans";
  CHECK(pinned.h == kPinned);
  if (g_failures) { std::printf("%ld of %ld checks FAILED\n", g_failures, g_checks); return 1; }
  std::printf("all checks passed (%ld)\n", g_checks);
  return 0;
}
