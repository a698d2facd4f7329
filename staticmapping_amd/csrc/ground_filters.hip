// ground_filters.hip -- kernels of GroundRemoval, GroundRemoval2 and RangeImage (included by cloud_filters.hip, which drives them).
//
// Reference: pre_processors/ of the reference
//   filter_ground_removal.cc:51-112    GroundRemoval   drop every voxel with fewer than min points, and the flat low ones
//   filter_ground_removal2.cc:134-377  GroundRemoval2  line fits along 180 angular segments ("fast segmentation of 3D point
//                                                     clouds for ground vehicles"); drop the points close to a line
//   filter_range_image.cc:75-155       RangeImage      keep the first point of every range-image pixel
// Every float expression is written operation by operation with contraction switched off: the reference is built without
// fused multiply-adds.  Angles are (float)atan2((double)y, (double)x) here and in the CPU restatement
// (tests/ground_filters_ref.py); the reference calls glibc's atan2f, which may differ by an ulp at a segment or pixel boundary.
// float -> int conversions follow x86's cvttss2si / cvttsd2si, which the reference runs on: truncation, and INT_MIN for NaN
// and for values outside the int range (trunc_x86).

__device__ __forceinline__ int trunc_x86(float v) { return (v >= -2147483648.f && v < 2147483648.f) ? (int)v : INT_MIN; }
__device__ __forceinline__ int trunc_x86(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : INT_MIN; }
__device__ __forceinline__ bool finite3(const float4 p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }
__device__ __forceinline__ float angle_f(float y, float x) { return (float)atan2((double)y, (double)x); }
// a correctly rounded float square root: __fsqrt_rn lowers to v_sqrt_f32 (1 ulp) on gfx950; the double root rounded to float
// is the float root (53 >= 2 * 24 + 2 bits)
__device__ __forceinline__ float sqrt_rn(float v) { return (float)sqrt((double)v); }
__device__ __forceinline__ float xy_range(const float4 p) {
#pragma clang fp contract(off)
  return sqrt_rn(p.x * p.x + p.y * p.y);                                   // std::sqrt(x * x + y * y), float
}

// ---- GroundRemoval2 ------------------------------------------------------------------------------
struct Gr2Args {
  float r_min, delta_alpha, delta_bin, two_pi;                             // SetInputCloud, :146-148
  float start_h, long_thr, long_h, start_max, max_err, max_slope, max_dist;
  int B, S, G, search_step;                                                // G = S * B grids; search_step: ClusterGround, :319-320
};

// SetInputCloud, :163-192.  `range < r_min_ && range > r_max_` is never true: every finite row is binned (clamped indices).
// Rows with a non-finite x, y or z get key G: never a grid member, never removed.
__global__ void gr2_bin(const float4* pts, int n, Gr2Args a, unsigned long long* keys, int32_t* idx) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  unsigned long long key = (unsigned long long)a.G;
  if (finite3(p)) {
    const float range = xy_range(p);
    float rad = angle_f(p.y, p.x);
    if (rad < 0.f) rad = rad + a.two_pi;
    int s = trunc_x86(rad / a.delta_alpha), b = trunc_x86((range - a.r_min) / a.delta_bin);
    if (b >= a.B) b = a.B - 1; else if (b < 0) b = 0;
    if (s >= a.S) s = a.S - 1; else if (s < 0) s = 0;
    key = (unsigned long long)s * (unsigned long long)a.B + (unsigned long long)b;
  }
  keys[i] = key;
  idx[i] = i;
}

// after the stable sort by grid: (d, z) per sorted position and the end of every grid's run
__global__ void gr2_gather(const float4* pts, const unsigned long long* skeys, const int32_t* sidx, int n, int G, float* gd, float* gz,
                           int32_t* gend) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const unsigned long long key = skeys[s];
  if (key >= (unsigned long long)G) { gd[s] = 0.f; gz[s] = 0.f; return; }
  const float4 p = pts[sidx[s]];
  gd[s] = xy_range(p);
  gz[s] = p.z;
  if (s == n - 1 || skeys[s + 1] != key) gend[key] = s + 1;
}

// :181-191 in input order: the grid's minimum is updated first (empty grid or z < min), then the point joins when
// z <= min + 0.5 (float min, double sum).  runmin = the segmented running minimum (inclusive, input order inside a grid), so
// membership is relative to the minimum so far.  min_z_point = the first point that reaches the grid's final minimum.
__global__ void gr2_mark(const unsigned long long* skeys, const float* gz, const float* runmin, const int32_t* gend, int n, int G,
                         int32_t* member, int32_t* gfirst) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const unsigned long long key = skeys[s];
  if (key >= (unsigned long long)G) { member[s] = 0; return; }
  const float z = gz[s];
  member[s] = ((double)z <= (double)runmin[s] + 0.5) ? 1 : 0;
  if (z == runmin[gend[key] - 1]) atomicMin(gfirst + key, s);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma clang fp contract(off)
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}

// FitLocalLine, :28-43 -- THE ONE UNPINNED STEP.  The reference solves [d 1] (m, b) = z with Eigen's colPivHouseholderQr in
// double and stores m, b as float.  Here: the centred normal equations in double, m = Sdz / Sdd, b = mean_z - m mean_d, every sum
// in one fixed order (lane j adds points j, j + 64, ... in turn, then a xor butterfly over the 64 lanes), which the CPU
// restatement repeats bit for bit.  It agrees with a least-squares solve to ~1e-15 relative on the lines seen here.
__device__ void gr2_fit(const float2* P, int L, int lane, float& m, float& b) {
#pragma clang fp contract(off)
  double sd = 0.0, sz = 0.0;
  for (int j = lane; j < L; j += 64) { sd = sd + (double)P[j].x; sz = sz + (double)P[j].y; }
  sd = wave_sum(sd); sz = wave_sum(sz);
  const double md = sd / (double)L, mz = sz / (double)L;
  double sdd = 0.0, sdz = 0.0;
  for (int j = lane; j < L; j += 64) {
    const double dd = (double)P[j].x - md, dz = (double)P[j].y - mz;
    sdd = sdd + dd * dd; sdz = sdz + dd * dz;
  }
  sdd = wave_sum(sdd); sdz = wave_sum(sdz);
  const double mm = sdz / sdd;
  m = (float)mm;
  b = (float)(mz - mm * md);
}

// GetMaxError, :45-55 (the maximum is exact in any order)
__device__ float gr2_max_error(const float2* P, int L, int lane, float m, float b) {
#pragma clang fp contract(off)
  float e = 0.f;
  for (int j = lane; j < L; j += 64) {
    const float err = fabsf(m * P[j].x + b - P[j].y);
    if (err > e) e = err;
  }
  for (int off = 32; off > 0; off >>= 1) { const float o = __shfl_xor(e, off); if (o > e) e = o; }
  return e;
}

// FitLines, :236-305: one wavefront per segment, serial over the bins; the current line's points live in LDS (bin_num float2),
// the lanes share its sums and GetMaxError.  Lines: (start d, start z, end d, end z) as LocalLineToLine makes them, :57-70.
__global__ __launch_bounds__(64) void gr2_fit_lines(const float* gd, const float* gz, const int32_t* gfirst, Gr2Args a, float4* lines,
                                                    int32_t* nlines) {
#pragma clang fp contract(off)
  extern __shared__ float2 P[];
  const int seg = blockIdx.x, lane = threadIdx.x, B = a.B;
  const int32_t* gf = gfirst + (size_t)seg * B;
  float4* out = lines + (size_t)seg * B;
  int start = 0;
  while (start < B && gf[start] == INT_MAX) ++start;
  int nl = 0;
  if (start < B - 1) {                                                     // :246-248
    float2 front = make_float2(gd[gf[start]], gz[gf[start]]), back = front;
    if (lane == 0) P[0] = front;
    __syncthreads();
    int L = 1;
    float cm = 0.f, cb = 0.f;                                              // LocalLine's defaults
    bool is_long = false;
    float gh = a.start_h;
    for (int i = start + 1; i < B; ++i) {
      const int f = gf[i];
      if (f == INT_MAX) continue;
      const float2 cp = make_float2(gd[f], gz[f]);
      if (cp.x - back.x >= a.long_thr) is_long = true;                    // :265-268
      float ez = FLT_MAX;
      if (is_long && L > 2) ez = cm * cp.x + cb;                           // :270-273
      if (L >= 2) {
        if (lane == 0) P[L] = cp;
        __syncthreads();
        ++L;
        gr2_fit(P, L, lane, cm, cb);                                       // current_line keeps this fit even when it fails
        const float err = gr2_max_error(P, L, lane, cm, cb);
        if (err > a.max_err || fabsf(cm) > a.max_slope || (is_long && fabsf(ez - cp.y) > a.long_h)) {
          --L;                                                             // pop_back: `back` is still the last point
          if (L >= 3) {
            float nm, nb;
            gr2_fit(P, L, lane, nm, nb);
            if (lane == 0) out[nl] = make_float4(front.x, nm * front.x + nb, back.x, nm * back.x + nb);
            ++nl;
            gh = nm * back.x + nb;                                         // :288-289
          }
          is_long = false;                                                 // a new line from the last point; the bin is visited again
          __syncthreads();
          if (lane == 0) P[0] = back;
          __syncthreads();
          front = back;
          L = 1;
          --i;
        } else {
          back = cp;
        }
      } else {
        if (!is_long && fabsf(back.y - gh) < a.start_max) {               // :297-304
          if (lane == 0) P[L] = cp;
          ++L;
        } else {
          if (lane == 0) P[0] = cp;
          front = cp;
          L = 1;
        }
        __syncthreads();
        back = cp;
      }
    }
    if (L > 2) {                                                           // :306-309
      float nm, nb;
      gr2_fit(P, L, lane, nm, nb);
      if (lane == 0) out[nl] = make_float4(front.x, nm * front.x + nb, back.x, nm * back.x + nb);
      ++nl;
    }
  }
  if (lane == 0) nlines[seg] = nl;
}

// VerticalDistanceToSegment, :379-397: every covering line overwrites the distance (the last one wins); -1 when none covers
__device__ float gr2_vdist(const float2 p, const float4* L, int nl) {
#pragma clang fp contract(off)
  const float margin = 0.1f;
  float dist = -1.f;
  for (int j = 0; j < nl; ++j) {
    const float4 l = L[j];
    if (l.x - margin < p.x && l.z + margin > p.x) {
      const float dz = l.w - l.y, dd = l.z - l.x;
      const float ez = (p.x - l.x) / dd * dz + l.y;
      dist = fabsf(p.y - ez);
    }
  }
  return dist;
}

// ClusterGround, :316-375: one thread per sorted point; members only; neighbours +k, -k for k = search_step .. 1, wrapping once
__global__ void gr2_cluster(const unsigned long long* skeys, const int32_t* sidx, const float* gd, const float* gz, const int32_t* member,
                            int n, Gr2Args a, const float4* lines, const int32_t* nlines, int32_t* flag) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const unsigned long long key = skeys[s];
  int keep = 1;
  if (key < (unsigned long long)a.G && member[s]) {
    const int seg = (int)(key / (unsigned long long)a.B);
    const float2 p = make_float2(gd[s], gz[s]);
    float dist = gr2_vdist(p, lines + (size_t)seg * a.B, nlines[seg]);
    if (dist < 0.f) {
      for (int k = a.search_step; k > 0; --k) {
        int c = seg + k;
        if (c >= a.S) c -= a.S;
        dist = gr2_vdist(p, lines + (size_t)c * a.B, nlines[c]);
        if (dist > 0.f) break;
        c = seg - k;
        if (c < 0) c += a.S;
        dist = gr2_vdist(p, lines + (size_t)c * a.B, nlines[c]);
        if (dist > 0.f) break;
      }
    }
    keep = (dist > 0.f && dist <= a.max_dist) ? 0 : 1;                     // a distance of exactly 0 is kept
  }
  flag[sidx[s]] = keep;
}

// ---- GroundRemoval -------------------------------------------------------------------------------
// voxel index static_cast<int>(coord / leaf): truncation towards zero, so voxel 0 spans (-leaf, leaf); 21 bits per axis.
// Non-finite rows get key ~0 (sorted last, kept).
__global__ void gr_keys(const float4* pts, int n, float leaf, unsigned long long* keys, int32_t* idx, int32_t* bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  unsigned long long key = ~0ull;
  if (finite3(p)) {
    const long a = (long)trunc_x86(p.x / leaf) + kVoxBias, b = (long)trunc_x86(p.y / leaf) + kVoxBias,
               c = (long)trunc_x86(p.z / leaf) + kVoxBias;
    if (a >= 0 && a < 2 * kVoxBias && b >= 0 && b < 2 * kVoxBias && c >= 0 && c < 2 * kVoxBias)
      key = ((unsigned long long)a << 42) | ((unsigned long long)b << 21) | (unsigned long long)c;
    else
      atomicAdd(bad, 1);
  }
  keys[i] = key;
  idx[i] = i;
}

// float <-> int with the same order (for atomicMin / atomicMax on z)
__device__ __forceinline__ int ford(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float fdeord(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__global__ void gr_minmax(const float4* pts, const unsigned long long* skeys, const int32_t* sidx, const int32_t* incl, int n,
                          int32_t* vmin, int32_t* vmax) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n || skeys[s] == ~0ull) return;
  const int v = incl[s] - 1, z = ford(pts[sidx[s]].z);
  atomicMin(vmin + v, z);
  atomicMax(vmax + v, z);
}

// Filter, :67-112: a voxel of fewer than min points disappears; a voxel of z index <= 0 whose z spread is in [0, height] is
// ground.  The reference's max / min start at -1e9 / 1e9.
__global__ void gr_flags(const unsigned long long* skeys, const int32_t* sidx, const int32_t* incl, const int32_t* start,
                         const int32_t* count, int n, float height, int min_pts, const int32_t* vmin, const int32_t* vmax, int32_t* flag) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const unsigned long long key = skeys[s];
  int keep = 1;
  if (key != ~0ull) {
    const int v = incl[s] - 1, V = count[0];
    const int size = (v + 1 < V ? start[v + 1] : n) - start[v];
    if (size < min_pts) {
      keep = 0;
    } else if ((long)(key & 0x1fffffull) - kVoxBias <= 0) {
      float mx = fdeord(vmax[v]), mn = fdeord(vmin[v]);
      if (!(mx > -1.e9f)) mx = -1.e9f;
      if (!(mn < 1.e9f)) mn = 1.e9f;
      const float delta = mx - mn;
      keep = (delta >= 0.f && delta <= height) ? 0 : 1;
    }
  }
  flag[sidx[s]] = keep;
}

// ---- RangeImage ----------------------------------------------------------------------------------
struct RiArgs {
  float ox, oy, oz, vres, hres;                                            // image_vertical_res / image_horizontal_res, :84-88
  double btm_rad;                                                          // btm_angle_ / 180.f * M_PI (double)
  int V, H;
};

// Filter, :95-121: the pixel of every row (-1 = dropped); the table keeps the smallest row index per pixel
__global__ void ri_pixel(const float4* pts, int n, RiArgs a, int32_t* pixel_of, int32_t* table) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  int pixel = -1;
  if (finite3(p)) {                                                        // non-finite rows are dropped
    const float x = p.x + a.ox, y = p.y + a.oy, z = p.z + a.oz;
    const float dxy = sqrt_rn(x * x + y * y);
    if (!(dxy < 0.01f)) {
      const float vr = angle_f(z, dxy);
      const int row = trunc_x86(((double)vr - a.btm_rad) / (double)a.vres);
      if (row >= 0 && row < a.V) {
        float hr = angle_f(y, x);
        if (hr < 0.f) hr = (float)((double)hr + M_PI * 2);
        int col = (int)lroundf(hr / a.hres);
        if (col >= a.H) col -= a.H;
        if (col >= 0 && col < a.H) pixel = row * a.H + col;
      }
    }
  }
  pixel_of[i] = pixel;
  if (pixel >= 0) atomicMin(table + pixel, i);
}

__global__ void ri_flags(const int32_t* pixel_of, const int32_t* table, int n, int32_t* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int px = pixel_of[i];
  flag[i] = (px >= 0 && table[px] == i) ? 1 : 0;
}
