// grid_sort_build.hip -- the ICP search grid of a small target built by ONE in-LDS sort per pair.
//
// Fragment of the ICP translation unit (smhip_api.hip includes it behind icp_kernels.hip, whose grid_setup_pair, centre_point and
// block_excl_scan it uses).  It produces, byte for byte, what grid_setup / grid_mark / grid_rank / grid_count / grid_cscan /
// grid_scatter_idx / grid_place produce for sort_cells = 1 without the row bitmap: PairState's mean, geometry and nocc,
// words[0..nw), cstart[0..nocc] and the cell-sorted tq / tn -- for targets of at most kGsMaxPoints points (plan::sorted_grid_build
// chooses).  The structure IS a stable sort of the points by cell key, so it is made as one: no bitmap to zero, no atomics, no
// arrival order to undo, none of bits / ccount / tcell / tslot / tord touched.
//
//   grid_sort_build   grid = (pairs), 1 024 threads.  Needs tgt_reduce to have run (its rows are folded in grid_setup's order).
//
// LDS of the workgroup (144 KiB of gfx950's 160 as compiled: the arrays below are 132 KiB, the compiler keeps grid_setup_pair's
// small private arrays there too):
//   s_buf  [32 768] u32   128 KiB  the sort's one buffer.  Pass 0 takes the keys from registers; every pass reads its elements into
//                                  registers before anybody scatters, so the scatter goes back into the same buffer.  An element is
//                                  (key >> 6) << 15 | caller index: the low six key bits are spent by pass 0 and computed again from
//                                  the point once the order is known, which is what lets 23 key bits + 15 index bits fit a word.
//                                  After the sort: the sorted full keys, then the occupied cells' keys, compacted (the fill reads them).
//   s_cnt  [64][16]   u32   4 KiB  digit counters, one column per wave; scanned digit-major they are the scatter offsets
//   s_w, s_g                       block_excl_scan's words, the pair's geometry (broadcast from the lane that ran grid_setup_pair)
#pragma once

namespace smhip {

constexpr int kGsThreads = 1024;
constexpr int kGsRounds = 32;                           // rounds of 64 consecutive elements a wave owns at most
constexpr int kGsMaxPoints = kGsThreads * kGsRounds;    // 32 768: the element's 15 index bits (and the shadow word's match field)
constexpr int kGsDigitBits = 6;                         // 64 digits x 16 waves = one counter per thread
constexpr int kGsIndexBits = 15;
constexpr int kGsFillWords = 8;                         // consecutive words a lane fills per search of the cell list (four 16-byte stores)

struct GsGeom {
  double mu[3];
  float origin[3];
  float inv_h;
  int32_t nx, ny, nz, wx, nw, nt;
};

// (word << 5) | bit of a centred point: grid_mark's arithmetic
__device__ __forceinline__ uint32_t gs_cell_key(const float3 c, const GsGeom& g) {
  int ix = (int)floorf((c.x - g.origin[0]) * g.inv_h);
  int iy = (int)floorf((c.y - g.origin[1]) * g.inv_h);
  int iz = (int)floorf((c.z - g.origin[2]) * g.inv_h);
  ix = min(max(ix, 0), g.nx - 1); iy = min(max(iy, 0), g.ny - 1); iz = min(max(iz, 0), g.nz - 1);
  const uint32_t w = (uint32_t)((iz * g.ny + iy) * g.wx + (ix >> 5));
  return (w << 5) | (uint32_t)(ix & 31);
}

// the lanes of the wave that hold the same digit as this one, among the valid ones (every lane of the wave calls it)
__device__ __forceinline__ unsigned long long gs_match(uint32_t digit, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int k = 0; k < kGsDigitBits; ++k) {
    const bool one = (digit >> k) & 1u;
    const unsigned long long bb = __ballot(one);
    m &= one ? bb : ~bb;
  }
  return m;
}

// One stable counting pass over six key bits.  Wave w owns the elements [w * chunk, (w + 1) * chunk) in rounds of 64 consecutive
// ones and a column of the counters.  Counting is an LDS add per element.  Placing: inside a round the lanes of one digit find each
// other (gs_match); their lowest lane takes the run's place from the wave's counter of that digit and hands it round, and each lane
// stands behind the lanes below it.  The order of the adds to a counter is the order of the wave's rounds, so the pass is stable.
// first: e[] holds full keys (nothing is read from s_buf) and the packed elements are formed on the way out.
__device__ __forceinline__ void gs_pass(uint32_t (&e)[kGsRounds], uint32_t* s_buf, uint32_t* s_cnt, uint32_t* s_w,
                                        int n, int chunk, int rounds, bool first, int shift) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  int base = wave * chunk + lane;
  s_cnt[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < kGsRounds; ++r) {
    if (r >= rounds) continue;
    const int pos = base + r * 64;
    if (pos < n) {
      if (!first) e[r] = s_buf[pos];
      atomicAdd(&s_cnt[((first ? e[r] : e[r] >> shift) & 63u) * 16 + wave], 1u);
    }
  }
  __syncthreads();
  uint32_t total;
  const uint32_t excl = block_excl_scan(s_cnt[threadIdx.x], s_w, &total);    // digit-major: digit d of wave 0, 1, ... then d + 1
  s_cnt[threadIdx.x] = excl;                                                   // (every element was read into e[] before this point)
  __syncthreads();
  // (a value the compiler cannot see through: it would otherwise keep the first loop's 32 positions and bounds tests alive for the
  // second one, and e[] needs those registers)
  asm volatile("" : "+v"(base));
#pragma unroll
  for (int r = 0; r < kGsRounds; ++r) {
    if (r >= rounds) continue;                                   // (uniform: the ballots below see whole waves)
    const int pos = base + r * 64;
    const bool valid = pos < n;
    const uint32_t d = valid ? (first ? e[r] : e[r] >> shift) & 63u : 0u;
    const unsigned long long m = gs_match(d, valid);
    const int leader = __ffsll((long long)m) - 1;
    uint32_t at = 0;
    if (valid && lane == leader) at = atomicAdd(&s_cnt[d * 16 + wave], (uint32_t)__popcll(m));
    at = (uint32_t)__shfl((int)at, leader & 63, 64);
    if (valid) s_buf[at + (uint32_t)__popcll(m & below)] = first ? ((e[r] >> kGsDigitBits) << kGsIndexBits) | (uint32_t)pos : e[r];   // < n: the counters sum to n
  }
  __syncthreads();
}

__global__ __launch_bounds__(kGsThreads) void grid_sort_build(IcpDev b) {
  __shared__ uint32_t s_buf[kGsMaxPoints];
  __shared__ uint32_t s_cnt[kGsThreads];
  __shared__ uint32_t s_w[17];
  __shared__ GsGeom s_g;
  const int pair = b.pair_base + blockIdx.x;
  PairState* st = &b.state[pair];
  if (threadIdx.x == 0) {
    grid_setup_pair(b, pair);
    for (int d = 0; d < 3; ++d) { s_g.mu[d] = st->mu[d]; s_g.origin[d] = st->origin[d]; }
    s_g.inv_h = st->inv_h;
    s_g.nx = st->nx; s_g.ny = st->ny; s_g.nz = st->nz; s_g.wx = st->wx; s_g.nw = st->nw;
    s_g.nt = min(max(b.in[pair].nt, 0), min(b.nt_cap, kGsMaxPoints));      // (the plan sends no larger target here)
  }
  __syncthreads();
  const GsGeom g = s_g;
  // (a non-finite target: grid_setup_pair left the one-cell placeholder geometry and the failed status; like the other form, the
  // build goes on over it -- every key clamps to cell 0)
  const int n = g.nt, nw = g.nw;
  const size_t o = (size_t)pair * b.nt_cap;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunk = ((n + 16 * 64 - 1) / (16 * 64)) * 64;        // elements per wave: whole rounds, at most kGsRounds of them
  const int rounds = chunk / 64;

  // ---- keys in caller order, then the sort: pass 0 on key bits [0, 6), the others on what the grid's size leaves
  uint32_t e[kGsRounds];
#pragma unroll
  for (int r = 0; r < kGsRounds; ++r) {
    const int pos = wave * chunk + r * 64 + lane;
    e[r] = r < rounds && pos < n ? gs_cell_key(centre_point(b.tgt_p[o + pos], g.mu), g) : 0u;
    if ((r & 7) == 7) __builtin_amdgcn_sched_barrier(0);         // eight 16-byte loads in flight, not thirty-two: e[] needs the registers
  }
  const int key_bits = 32 - __clz((((uint32_t)nw - 1u) << 5) | 31u);
#pragma unroll 1
  for (int done = 0; done == 0 || done < key_bits; done += kGsDigitBits)
    gs_pass(e, s_buf, s_cnt, s_w, n, chunk, rounds, done == 0, kGsIndexBits + done - kGsDigitBits);

  // ---- the sorted target, written in order; the element gives way to the point's full key
  float4* tq = b.tq + o;
  float4* tn = b.tn + o;
  for (int i = threadIdx.x; i < n; i += kGsThreads) {
    const uint32_t j = s_buf[i] & ((1u << kGsIndexBits) - 1u);
    const float3 c = centre_point(b.tgt_p[o + j], g.mu);
    float4 nn = b.tgt_n[o + j];
    nn.w = 0.f;
    tq[i] = make_float4(c.x, c.y, c.z, __int_as_float((int)j));
    tn[i] = nn;
    s_buf[i] = gs_cell_key(c, g);
  }
  __syncthreads();

  // ---- run boundaries: cstart, nocc, and the occupied cells' keys compacted to the front of s_buf
  const int per = (n + kGsThreads - 1) / kGsThreads;             // <= kGsRounds
  const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
  uint32_t before = 0xffffffffu, cells = 0;
  if (lo > 0 && lo < hi) before = s_buf[lo - 1];
#pragma unroll
  for (int q = 0; q < kGsRounds; ++q) {
    if (lo + q < hi) {
      e[q] = s_buf[lo + q];
      cells += e[q] != (q == 0 ? before : e[q - 1]) ? 1u : 0u;
    }
  }
  uint32_t nocc;
  uint32_t c = block_excl_scan(cells, s_w, &nocc);               // (its barriers stand between the loads above and the stores below)
  uint32_t* cs = b.cstart + (size_t)pair * (b.nt_cap + 1);
#pragma unroll
  for (int q = 0; q < kGsRounds; ++q) {
    if (lo + q < hi && e[q] != (q == 0 ? before : e[q - 1])) {
      cs[c] = (uint32_t)(lo + q);
      s_buf[c] = e[q];                                           // c <= lo + q
      ++c;
    }
  }
  if (threadIdx.x == 0) { cs[nocc] = (uint32_t)n; st->nocc = (int)nocc; }
  __syncthreads();

  // ---- words[0..nw): a lane takes kGsFillWords consecutive words, finds the first cell at or behind them with one binary search
  // in the compacted keys, and walks on from there; the rank of a word is the position of that cell
  uint2* words = b.words + (size_t)pair * kMaxGridWords;
  uint32_t from = 0;
  for (int w0 = (int)threadIdx.x * kGsFillWords; w0 < nw; w0 += kGsThreads * kGsFillWords) {
    uint32_t a = from, z = nocc;
    const uint32_t want = (uint32_t)w0 << 5;
    while (a < z) {
      const uint32_t mid = (a + z) >> 1;
      if (s_buf[mid] < want) a = mid + 1; else z = mid;
    }
    from = a;
    uint2 out[kGsFillWords];
#pragma unroll
    for (int k = 0; k < kGsFillWords; ++k) {
      uint32_t bits = 0;
      const uint32_t rank = a;
      while (a < nocc && (s_buf[a] >> 5) == (uint32_t)(w0 + k)) { bits |= 1u << (s_buf[a] & 31u); ++a; }
      out[k] = make_uint2(bits, rank);
    }
    if (w0 + kGsFillWords <= nw) {
#pragma unroll
      for (int k = 0; k < kGsFillWords; k += 2)                  // kMaxGridWords and w0 keep these 16-byte aligned
        *reinterpret_cast<uint4*>(words + w0 + k) = make_uint4(out[k].x, out[k].y, out[k + 1].x, out[k + 1].y);
    } else {
#pragma unroll
      for (int k = 0; k < kGsFillWords; ++k) if (w0 + k < nw) words[w0 + k] = out[k];
    }
  }
}

}  // namespace smhip
