// statistic_removal.hip -- kernels of StatisticRemoval (included by cloud_filters.hip, which drives them).
//
// Reference: pre_processors/filter_statistic_removal.cc of the reference.  :31-37 give the two parameters and their defaults;
// Filter (:44-59) holds only a commented-out pcl::StatisticalOutlierRemoval call (setMeanK, setStddevMulThresh) and a TODO, so
// what is computed here is this project's definition ("StatisticRemoval"; restated in
// tests/statistic_removal_ref.py): the PCL 1.8 algorithm with every float and double operation and its order fixed.
//
//   d2(a, b) = ((dx*dx) + (dy*dy)) + (dz*dz) in float, every operation rounded on its own (no fused multiply-add)
//   distance[i] = (float)(sum of sqrt((double)d2) over the k smallest d2 of row i, ascending, in double) / k)
//   a row is removed iff it is finite and (double)distance[i] > mean + std_mul * stddev of the finite rows' distances
//
// The search structure is the cloud sorted along ONE axis (the longest side of the finite rows' bounding box), not a grid of
// cells: a query walks outwards from its own place in the sorted order, to the left and to the right, and a side ends at the
// first row whose squared offset along the axis, da2 = fl(fl(q.a - c.a)^2), exceeds the largest d2 of the best-k set.  That bound
// holds for the float d2 as computed, not only for the real distance: da2 is one of the three products of d2, the other two
// are >= 0, and a rounded sum of non-negative floats is never below either operand, so d2 >= da2; and along a sorted side
// |fl(q.a - c.a)| never shrinks (rounding is monotone), so every later row of that side is excluded as well.  There is no cell
// size, no coordinate range and nothing approximate: an isolated row simply walks further (at worst over the whole cloud).
// The multiset of the k smallest d2 does not depend on how ties are broken, so the answer is a function of the rows alone --
// not of the axis, the sort or the walk.

constexpr int kSrThreads = 128;
constexpr int kSrMaxK = 64;                      // the best-k set of a query lives in LDS: KMAX x 128 threads x 4 B <= 32 KiB

// floats in an order unsigned integers keep (-0.0 sorts before +0.0; both are the same coordinate)
__device__ __forceinline__ uint32_t sr_ordered(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// meta[0..2] = min x y z, meta[3..5] = max x y z of the finite rows (as sr_ordered words), meta[6] = V, the number of finite
// rows.  Integer minima, maxima and counts: the result does not depend on the order the waves arrive in.  Launched with few
// workgroups striding over the rows: seven atomics per wave on the same words, so the fewer waves the better.
__global__ void sr_extent(const float4* pts, int n, uint32_t* meta) {
  uint32_t lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  int cnt = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float4 p = pts[i];
    if (!finite3(p)) continue;
    const float c[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], sr_ordered(c[a])); hi[a] = max(hi[a], sr_ordered(c[a])); }
    ++cnt;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], off));
      hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], off));
    }
    cnt += __shfl_xor(cnt, off);
  }
  if ((threadIdx.x & 63) == 0 && cnt > 0) {
    for (int a = 0; a < 3; ++a) { atomicMin(&meta[a], lo[a]); atomicMax(&meta[3 + a], hi[a]); }
    atomicAdd(&meta[6], (uint32_t)cnt);
  }
}

// sort key = the coordinate along `axis`; non-finite rows get the largest key and so end up behind the V finite ones
__global__ void sr_keys(const float4* pts, int n, int axis, unsigned long long* keys, int32_t* idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  const float a = axis == 0 ? p.x : (axis == 1 ? p.y : p.z);
  keys[i] = finite3(p) ? (unsigned long long)sr_ordered(a) : 0xFFFFFFFFull;   // sr_ordered(FLT_MAX) = 0xFF7FFFFF
  idx[i] = i;
}

// the finite rows in sorted order, the sort coordinate repeated in w
__global__ void sr_gather(const float4* pts, const int32_t* sidx, int V, int axis, float4* sp) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= V) return;
  const float4 p = pts[sidx[s]];
  sp[s] = make_float4(p.x, p.y, p.z, axis == 0 ? p.x : (axis == 1 ? p.y : p.z));
}

// One query per thread (sorted position s), its best-k set in LDS as an UNSORTED set of distances plus, in registers, the
// largest member and the slot that holds it (what gicp_knn_cov learnt: a sorted list shifts half its entries through LDS on
// every accepted candidate).  Only the distances are kept: the result needs no neighbour indices, and ties need no rule.
// Slots >= k hold -2 and never become the largest.  The walk takes four rows of a side at a time so that four loads are in
// flight; the threads of a wave are neighbours along the axis and read nearly the same rows.
template <int KMAX>
__global__ __launch_bounds__(kSrThreads) void sr_knn(const float4* sp, const int32_t* sidx, int V, int n, int k, float* dist) {
#pragma clang fp contract(off)
  __shared__ float s_d[KMAX][kSrThreads];
  const int t = threadIdx.x, s = blockIdx.x * kSrThreads + t;
  if (s >= n) return;
  if (s >= V) { dist[sidx[s]] = 0.f; return; }                 // a non-finite row: distance 0, no one's neighbour
  const float4 q = sp[s];
#pragma unroll
  for (int m = 0; m < KMAX; ++m) s_d[m][t] = m < k ? INFINITY : -2.0f;
  float worst = INFINITY;
  int wpos = 0;
  // false = this row ends its side; true = it was weighed against the set
  auto step = [&](const float4 c) -> bool {
    const float da = q.w - c.w;
    if (da * da > worst) return false;
    const float dx = q.x - c.x, dy = q.y - c.y, dz = q.z - c.z;
    const float d = ((dx * dx) + (dy * dy)) + (dz * dz);
    if (d < worst) {
      s_d[wpos][t] = d;                                          // evict the farthest member
      float dm[KMAX];
#pragma unroll
      for (int m = 0; m < KMAX; ++m) dm[m] = s_d[m][t];          // KMAX independent LDS reads, then the new farthest
      float w = -1.f;
      int wp = 0;
#pragma unroll
      for (int m = 0; m < KMAX; ++m) { const bool g = dm[m] > w; w = g ? dm[m] : w; wp = g ? m : wp; }
      worst = w; wpos = wp;
    }
    return true;
  };
  int lo = s - 1, hi = s + 1;
  bool L = lo >= 0, R = hi < V;
  while (L || R) {
    if (L) {
      const float4 c0 = sp[lo], c1 = sp[max(lo - 1, 0)], c2 = sp[max(lo - 2, 0)], c3 = sp[max(lo - 3, 0)];
      L = step(c0) && lo - 1 >= 0 && step(c1) && lo - 2 >= 0 && step(c2) && lo - 3 >= 0 && step(c3) && lo - 4 >= 0;
      lo -= 4;
    }
    if (R) {
      const float4 c0 = sp[hi], c1 = sp[min(hi + 1, V - 1)], c2 = sp[min(hi + 2, V - 1)], c3 = sp[min(hi + 3, V - 1)];
      R = step(c0) && hi + 1 < V && step(c1) && hi + 2 < V && step(c2) && hi + 3 < V && step(c3) && hi + 4 < V;
      hi += 4;
    }
  }
  // the ascending double sum without sorting: each pass takes the smallest value above the last one and adds its root as many
  // times as it occurs (V > k, so the set is full; a member at +inf -- an overflowed d2 -- is summed like any other)
  double sum = 0.0;
  float last = -1.f;
  for (int done = 0; done < k;) {
    float v = INFINITY;
    int c = 0;
#pragma unroll
    for (int m = 0; m < KMAX; ++m) {
      const float d = s_d[m][t];
      if (m < k && d > last) { if (d < v) { v = d; c = 1; } else if (d == v) ++c; }
    }
    if (c == 0) break;
    const double r = sqrt((double)v);
    for (int e = 0; e < c; ++e) sum += r;
    done += c;
    last = v;
  }
  dist[sidx[s]] = (float)(sum / (double)k);
}

// The two sums of step 6 in a fixed order that is a function of the row order alone.  Rows are taken in chunks of 64
// consecutive rows (a non-finite row adds its distance 0, which changes nothing); a chunk is folded by halving: the 64 values
// become 32 by v[l] + v[l + 32], then 16 by v[l] + v[l + 16], and so on down to one (sr_fold64).  The chunk sums are then dealt
// to 64 columns, chunk c to column c mod 64, each column summed in ascending c from 0.0, and the 64 column sums folded the
// same way.  The squares (double)d * (double)d are exact.
__device__ __forceinline__ double sr_fold64(double v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off);
  return v;                                                       // lane 0 holds the fold
}
__global__ void sr_chunk_sums(const float* dist, int n, double* csum, double* csq) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;             // blockDim.x is a multiple of 64: a wave = a chunk
  const double d = i < n ? (double)dist[i] : 0.0;
  const double a = sr_fold64(d), b = sr_fold64(d * d);
  if ((threadIdx.x & 63) == 0 && i < n) { csum[i >> 6] = a; csq[i >> 6] = b; }
}
// one wave: stats = sum, sq_sum, V, threshold
__global__ void sr_stats(const double* csum, const double* csq, int chunks, int V, float std_mul, double* stats) {
#pragma clang fp contract(off)
  double a = 0.0, b = 0.0;
  for (int c = threadIdx.x; c < chunks; c += 64) { a = a + csum[c]; b = b + csq[c]; }
  a = sr_fold64(a);
  b = sr_fold64(b);
  if (threadIdx.x != 0) return;
  const double v = (double)V;
  const double mean = a / v;
  const double variance = (b - a * a / v) / (v - 1.0);
  const double stddev = sqrt(variance);
  const double prod = (double)std_mul * stddev;
  stats[0] = a; stats[1] = b; stats[2] = v; stats[3] = mean + prod;
}
// keep = 1 unless the row is finite and farther than the threshold (a NaN threshold removes nothing)
__global__ void sr_flags(const float4* pts, const float* dist, int n, const double* stats, int32_t* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flag[i] = (finite3(pts[i]) && (double)dist[i] > stats[3]) ? 0 : 1;
}
