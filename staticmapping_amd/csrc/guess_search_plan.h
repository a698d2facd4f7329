// guess_search_plan.h -- the host side of the correlative guess search (DESIGN.md §6 "Guess search"): what a call is refused for
// from its sizes alone, the candidate volume, the bitmap over the target's voxel box, the packed source voxel, the yaw transforms
// and the pick rule.  No device call in it: everything here runs on the host (tests/cpp/test_guess_search_plan.cc), and the kernels
// (guess_search.hip) compile the layout and order functions marked SMHIP_GS_HD for the device as well, so both sides share one text.
//
//   candidates      (2 Ky + 1) x (2 half_z + 1) x (2 half_xy + 1)^2, flat index ((a + Ky) * nz + (k + half_z)) * nxy * nxy +
//                   (j + half_xy) * nxy + (i + half_xy): i runs fastest, one int32 of the score volume each
//   bitmap          bit x of row (z, y): word (z * ny + y) * row_words + (x >> 5), bit x & 31, x / y / z relative to the box origin
//   packed voxel    one 64-bit word per sampled source point and yaw: three 21-bit fields x | y << 21 | z << 42, each the
//                   coordinate relative to the box origin plus 2^20.  A point no offset of the window can bring into the box is
//                   stored as kNeverVoxel (every field 0: x = -2^20, which no offset below 2^19 lifts to 0)
//   pick            highest score; among equals the smallest i^2 + j^2 + k^2, then the smallest |a|, then the smallest a, k, j, i
#ifndef SMHIP_GUESS_SEARCH_PLAN_H_
#define SMHIP_GUESS_SEARCH_PLAN_H_

#include <cmath>
#include <cstdint>
#include <string>

#ifdef __HIPCC__
#define SMHIP_GS_HD __host__ __device__
#else
#define SMHIP_GS_HD
#endif

namespace smhip_guess_search {

constexpr long long kMaxCandidates = 1LL << 25;      // the score volume is one int32 per candidate
constexpr long long kMaxBitmapBits = 1LL << 28;
constexpr int kMaxHalf = 1 << 19;                    // a window offset; with the box extent it has to fit a packed field
constexpr int kFieldBias = 1 << 20, kFieldBits = 21;
constexpr int kMaxVoxel = 1 << 30;                   // |floor(p / res)| below this fits the index type
constexpr uint64_t kNeverVoxel = 0;

enum Refusal { kOk = 0, kInvalid = 1, kCapacity = 2 };

struct Window {
  int half_xy = 0, half_z = 0, yaw_steps = 0;
  int nxy = 1, nz = 1, nyaw = 1;
  long long n_offsets = 1, n_candidates = 1;         // offsets of one yaw; all of them
};

struct Bitmap {
  int origin[3] = {0, 0, 0}, extent[3] = {0, 0, 0};
  int row_words = 0;
  long long words = 0;
};

// the sizes alone: everything smhip_guess_search_f32 refuses before it touches anything
inline Refusal Check(bool pointers_ok, int target_stride, int source_stride, long long n_target, long long n_source, double res, int half_xy,
                     int half_z, int yaw_steps, double yaw_step, long long max_source_points, const double* guess16, long long max_points,
                     Window* w, std::string* why) {
  if (!pointers_ok) { *why = "null pointer"; return kInvalid; }
  if ((target_stride != 4 && target_stride != 5) || (source_stride != 4 && source_stride != 5)) {
    *why = "a stride other than 4 (x y z intensity) or 5 (InnerPointType)"; return kInvalid;
  }
  if (n_target < 1 || n_source < 1) { *why = "a cloud with no row"; return kInvalid; }
  if (!std::isfinite(res) || !(res > 0.0)) { *why = "resolution must be finite and positive"; return kInvalid; }
  if (half_xy < 0 || half_z < 0 || yaw_steps < 0) { *why = "a negative window"; return kInvalid; }
  if (!std::isfinite(yaw_step)) { *why = "yaw_step must be finite"; return kInvalid; }
  if (max_source_points < 1) { *why = "max_source_points must be at least 1"; return kInvalid; }
  for (int e = 0; e < 16; ++e)
    if (!std::isfinite(guess16[e])) { *why = "the guess is not finite"; return kInvalid; }
  if (half_xy > kMaxHalf || half_z > kMaxHalf || yaw_steps > kMaxHalf) { *why = "a window half-width above 2^19"; return kCapacity; }
  Window v;
  v.half_xy = half_xy; v.half_z = half_z; v.yaw_steps = yaw_steps;
  v.nxy = 2 * half_xy + 1; v.nz = 2 * half_z + 1; v.nyaw = 2 * yaw_steps + 1;
  v.n_offsets = static_cast<long long>(v.nxy) * v.nxy;                  // <= 2^40
  if (v.n_offsets > kMaxCandidates) { *why = "more than 2^25 candidates"; return kCapacity; }
  v.n_offsets *= v.nz;                                                  // <= 2^45
  if (v.n_offsets > kMaxCandidates) { *why = "more than 2^25 candidates"; return kCapacity; }
  v.n_candidates = v.n_offsets * v.nyaw;                                // <= 2^45
  if (v.n_candidates > kMaxCandidates) { *why = "more than 2^25 candidates"; return kCapacity; }
  if (n_target > max_points || n_source > max_points) { *why = "a cloud larger than the handle's capacity"; return kCapacity; }
  *w = v;
  return kOk;
}

// the bitmap over the target's voxel box [lo, hi] (inclusive, each |coordinate| < kMaxVoxel), for a window of these half-widths
inline Refusal MakeBitmap(const int lo[3], const int hi[3], int half_xy, int half_z, Bitmap* b, std::string* why) {
  Bitmap m;
  for (int c = 0; c < 3; ++c) {
    const long long e = static_cast<long long>(hi[c]) - lo[c] + 1;
    const int half = c == 2 ? half_z : half_xy;
    if (e < 1) { *why = "an empty voxel box"; return kInvalid; }
    if (e + half > kFieldBias) { *why = "the target's voxel box and the window do not fit a packed voxel field (2^20)"; return kCapacity; }
    m.origin[c] = lo[c]; m.extent[c] = static_cast<int>(e);
  }
  m.row_words = (m.extent[0] + 31) / 32;
  const long long rows = static_cast<long long>(m.extent[1]) * m.extent[2];       // < 2^40
  if (rows > kMaxBitmapBits || rows * m.row_words * 32 > kMaxBitmapBits) { *why = "a bitmap above 2^28 bits"; return kCapacity; }
  m.words = rows * m.row_words;
  *b = m;
  return kOk;
}

// rel = voxel - origin per axis, each in [-kFieldBias, kFieldBias)
SMHIP_GS_HD inline uint64_t PackVoxel(int rx, int ry, int rz) {
  return static_cast<uint64_t>(rx + kFieldBias) | (static_cast<uint64_t>(ry + kFieldBias) << kFieldBits) |
         (static_cast<uint64_t>(rz + kFieldBias) << (2 * kFieldBits));
}
SMHIP_GS_HD inline void UnpackVoxel(uint64_t v, int* rx, int* ry, int* rz) {
  constexpr uint64_t mask = (1ull << kFieldBits) - 1;
  *rx = static_cast<int>(v & mask) - kFieldBias;
  *ry = static_cast<int>((v >> kFieldBits) & mask) - kFieldBias;
  *rz = static_cast<int>((v >> (2 * kFieldBits)) & mask) - kFieldBias;
}
// can any offset of the window bring the relative voxel into the box?
inline bool Reachable(long long rx, long long ry, long long rz, const Bitmap& b, int half_xy, int half_z) {
  return rx >= -half_xy && rx < static_cast<long long>(b.extent[0]) + half_xy && ry >= -half_xy && ry < static_cast<long long>(b.extent[1]) + half_xy &&
         rz >= -half_z && rz < static_cast<long long>(b.extent[2]) + half_z;
}

// rows 0..2 of Rz(angle) * R0 and t0 as 12 doubles (r00 r01 r02 r10 .. r22 tx ty tz); guess16 is column-major.  Every product
// and sum rounded on its own, so that the numpy restatement forms the same doubles.
inline void YawTransform(const double* guess16, double angle, double* out12) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double c = std::cos(angle), s = std::sin(angle);
  for (int col = 0; col < 3; ++col) {
    const double r0 = guess16[4 * col], r1 = guess16[4 * col + 1], r2 = guess16[4 * col + 2];
    const double a = c * r0, b = s * r1, d = s * r0, e = c * r1;
    out12[col] = a - b;
    out12[3 + col] = d + e;
    out12[6 + col] = r2;
  }
  out12[9] = guess16[12]; out12[10] = guess16[13]; out12[11] = guess16[14];
}

struct Candidate { int a = 0, i = 0, j = 0, k = 0; };

SMHIP_GS_HD inline Candidate Decode(long long flat, const Window& w) {
  Candidate c;
  c.i = static_cast<int>(flat % w.nxy) - w.half_xy; flat /= w.nxy;
  c.j = static_cast<int>(flat % w.nxy) - w.half_xy; flat /= w.nxy;
  c.k = static_cast<int>(flat % w.nz) - w.half_z; flat /= w.nz;
  c.a = static_cast<int>(flat) - w.yaw_steps;
  return c;
}
SMHIP_GS_HD inline long long Encode(const Candidate& c, const Window& w) {
  return ((static_cast<long long>(c.a + w.yaw_steps) * w.nz + (c.k + w.half_z)) * w.nxy + (c.j + w.half_xy)) * w.nxy + (c.i + w.half_xy);
}

// rule 7: is (score_x, x) picked before (score_y, y)?  A total order on distinct candidates.
SMHIP_GS_HD inline bool Better(int score_x, const Candidate& x, int score_y, const Candidate& y) {
  if (score_x != score_y) return score_x > score_y;
  const long long dx = static_cast<long long>(x.i) * x.i + static_cast<long long>(x.j) * x.j + static_cast<long long>(x.k) * x.k;
  const long long dy = static_cast<long long>(y.i) * y.i + static_cast<long long>(y.j) * y.j + static_cast<long long>(y.k) * y.k;
  if (dx != dy) return dx < dy;
  const int ax = x.a < 0 ? -x.a : x.a, ay = y.a < 0 ? -y.a : y.a;
  if (ax != ay) return ax < ay;
  if (x.a != y.a) return x.a < y.a;
  if (x.k != y.k) return x.k < y.k;
  if (x.j != y.j) return x.j < y.j;
  return x.i < y.i;
}
// is y far enough from the pick x to count for runner_up_score?
SMHIP_GS_HD inline bool Apart(const Candidate& x, const Candidate& y) {
  const int di = y.i - x.i, dj = y.j - x.j, dk = y.k - x.k, da = y.a - x.a;
  return di > 2 || di < -2 || dj > 2 || dj < -2 || dk > 2 || dk < -2 || da > 1 || da < -1;
}

// the host's pick from a stored volume (what guess_search_pick does on the device): *best = the flat index
inline void Pick(const int32_t* volume, const Window& w, long long* best, int* runner_up) {
  long long b = 0;
  Candidate cb = Decode(0, w);
  for (long long f = 1; f < w.n_candidates; ++f) {
    if (volume[f] < volume[b]) continue;
    const Candidate c = Decode(f, w);
    if (Better(volume[f], c, volume[b], cb)) { b = f; cb = c; }
  }
  int r = 0;
  for (long long f = 0; f < w.n_candidates; ++f)
    if (volume[f] > r && Apart(cb, Decode(f, w))) r = volume[f];
  *best = b; *runner_up = r;
}

// rows kept of n finite source rows: all of them when n <= M, else floor(k n / M), k = 0 .. M - 1
inline long long SampleCount(long long n, long long M) { return n <= M ? n : M; }
inline long long SampleRow(long long k, long long n, long long M) { return n <= M ? k : (k * n) / M; }

}  // namespace smhip_guess_search
#endif  // SMHIP_GUESS_SEARCH_PLAN_H_
