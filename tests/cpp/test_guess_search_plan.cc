// staticmapping_amd/csrc/guess_search_plan.h on the host: every refusal, the candidate and bitmap sizes at and one past each limit,
// the packed voxel layout, the sample rule, the yaw transform and the pick rule on hand-made volumes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../staticmapping_amd/csrc/guess_search_plan.h"

namespace gs = smhip_guess_search;

static int g_failed = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #c); ++g_failed; } } while (0)

struct Args {
  bool pointers = true;
  int ts = 4, ss = 5;
  long long nt = 100, ns = 100;
  double res = 0.5;
  int hxy = 20, hz = 2, ky = 10;
  double step = 0.03;
  long long M = 4096;
  double guess[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  long long max_points = 1 << 18;
};
static gs::Refusal Run(const Args& a, gs::Window* w = nullptr) {
  gs::Window local;
  std::string why;
  const gs::Refusal r = gs::Check(a.pointers, a.ts, a.ss, a.nt, a.ns, a.res, a.hxy, a.hz, a.ky, a.step, a.M, a.guess, a.max_points, w ? w : &local, &why);
  EXPECT((r == gs::kOk) == why.empty());
  return r;
}

static void Refusals() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  gs::Window w;
  EXPECT(Run(Args(), &w) == gs::kOk);
  EXPECT(w.nxy == 41 && w.nz == 5 && w.nyaw == 21 && w.n_offsets == 8405 && w.n_candidates == 176505);      // the defaults
  { Args a; a.pointers = false; EXPECT(Run(a) == gs::kInvalid); }
  for (int s : {0, 3, 6, -4}) { Args a; a.ts = s; EXPECT(Run(a) == gs::kInvalid); Args b; b.ss = s; EXPECT(Run(b) == gs::kInvalid); }
  { Args a; a.ts = 5; a.ss = 4; EXPECT(Run(a) == gs::kOk); }
  { Args a; a.nt = 0; EXPECT(Run(a) == gs::kInvalid); a.nt = 1; EXPECT(Run(a) == gs::kOk); }
  { Args a; a.ns = 0; EXPECT(Run(a) == gs::kInvalid); a.ns = -3; EXPECT(Run(a) == gs::kInvalid); }
  for (double r : {0.0, -0.5, inf, nan}) { Args a; a.res = r; EXPECT(Run(a) == gs::kInvalid); }
  { Args a; a.hxy = -1; EXPECT(Run(a) == gs::kInvalid); }
  { Args a; a.hz = -1; EXPECT(Run(a) == gs::kInvalid); }
  { Args a; a.ky = -1; EXPECT(Run(a) == gs::kInvalid); }
  { Args a; a.hxy = a.hz = a.ky = 0; EXPECT(Run(a, &w) == gs::kOk); EXPECT(w.n_candidates == 1); }
  for (double s : {inf, nan}) { Args a; a.step = s; EXPECT(Run(a) == gs::kInvalid); }
  { Args a; a.M = 0; EXPECT(Run(a) == gs::kInvalid); a.M = 1; EXPECT(Run(a) == gs::kOk); }
  for (int e = 0; e < 16; ++e) { Args a; a.guess[e] = e % 2 ? nan : -inf; EXPECT(Run(a) == gs::kInvalid); }
  // capacity: the clouds at and one past the handle's size
  { Args a; a.nt = a.max_points; a.ns = a.max_points; EXPECT(Run(a) == gs::kOk); a.nt += 1; EXPECT(Run(a) == gs::kCapacity); }
  { Args a; a.ns = a.max_points + 1; EXPECT(Run(a) == gs::kCapacity); }
  // candidates: products of odd numbers, so the largest volume of one factor is 5791^2 = 33 535 681 <= 2^25 < 5793^2
  { Args a; a.hz = a.ky = 0; a.hxy = 2895; EXPECT(Run(a, &w) == gs::kOk); EXPECT(w.n_candidates == 33535681LL); a.hxy = 2896; EXPECT(Run(a) == gs::kCapacity); }
  // all four factors: 63^2 x 65 x 129 = 33280065 fits, 63^2 x 65 x 131 = 33796035 does not
  { Args a; a.hxy = 31; a.hz = 32; a.ky = 64; EXPECT(Run(a, &w) == gs::kOk); EXPECT(w.n_candidates == 33280065LL); a.ky = 65; EXPECT(Run(a) == gs::kCapacity); }
  { Args a; a.hxy = 0; a.hz = gs::kMaxHalf; a.ky = 0; EXPECT(Run(a) == gs::kOk); a.hz += 1; EXPECT(Run(a) == gs::kCapacity); }
  { Args a; a.hxy = 0; a.hz = 0; a.ky = gs::kMaxHalf; EXPECT(Run(a, &w) == gs::kOk); EXPECT(w.nyaw == 2 * gs::kMaxHalf + 1); a.ky += 1; EXPECT(Run(a) == gs::kCapacity); }
  { Args a; a.hxy = 1 << 30; EXPECT(Run(a) == gs::kCapacity); }                                               // no overflow on the way
  // invalid wins over capacity
  { Args a; a.hxy = 1 << 30; a.res = 0; EXPECT(Run(a) == gs::kInvalid); }
}

static void Bitmaps() {
  gs::Bitmap b;
  std::string why;
  { const int lo[3] = {-7, 2, -1}, hi[3] = {-7, 2, -1}; EXPECT(gs::MakeBitmap(lo, hi, 0, 0, &b, &why) == gs::kOk);
    EXPECT(b.extent[0] == 1 && b.extent[1] == 1 && b.extent[2] == 1 && b.row_words == 1 && b.words == 1 && b.origin[0] == -7 && b.origin[2] == -1); }
  for (int e : {31, 32, 33, 64, 65}) {
    const int lo[3] = {-40, 0, 0}, hi[3] = {-40 + e - 1, 2, 1};
    EXPECT(gs::MakeBitmap(lo, hi, 3, 1, &b, &why) == gs::kOk);
    EXPECT(b.row_words == (e + 31) / 32 && b.words == 6LL * ((e + 31) / 32));
  }
  // 1024 x 512 x 512 bits = 2^28: fits; one more layer, row or word does not
  { const int lo[3] = {0, 0, 0}; int hi[3] = {1023, 511, 511}; EXPECT(gs::MakeBitmap(lo, hi, 1, 1, &b, &why) == gs::kOk); EXPECT(b.words == (1LL << 23));
    hi[2] = 512; EXPECT(gs::MakeBitmap(lo, hi, 1, 1, &b, &why) == gs::kCapacity);
    hi[2] = 511; hi[1] = 512; EXPECT(gs::MakeBitmap(lo, hi, 1, 1, &b, &why) == gs::kCapacity);
    hi[1] = 511; hi[0] = 1024; EXPECT(gs::MakeBitmap(lo, hi, 1, 1, &b, &why) == gs::kCapacity); }       // (a row is padded to whole words)
  // the packed field: extent + half-width <= 2^20, per axis
  { const int lo[3] = {-5, 0, 0}; int hi[3] = {-5 + (1 << 20) - 3 - 1, 0, 0}; EXPECT(gs::MakeBitmap(lo, hi, 3, 0, &b, &why) == gs::kOk);
    EXPECT(gs::MakeBitmap(lo, hi, 4, 0, &b, &why) == gs::kCapacity); }
  { const int lo[3] = {0, 0, 10}; int hi[3] = {0, 0, 10 + (1 << 20) - 8 - 1}; EXPECT(gs::MakeBitmap(lo, hi, 100, 8, &b, &why) == gs::kOk);
    EXPECT(gs::MakeBitmap(lo, hi, 100, 9, &b, &why) == gs::kCapacity); }
  // the widest coordinates the kernels let through
  { const int lo[3] = {-(gs::kMaxVoxel - 1), 0, 0}, hi[3] = {gs::kMaxVoxel - 1, 0, 0}; EXPECT(gs::MakeBitmap(lo, hi, 0, 0, &b, &why) == gs::kCapacity); }
  { const int lo[3] = {1, 0, 0}, hi[3] = {0, 0, 0}; EXPECT(gs::MakeBitmap(lo, hi, 0, 0, &b, &why) == gs::kInvalid); }
}

static void Packing() {
  EXPECT(gs::PackVoxel(0, 0, 0) == ((1ull << 20) | (1ull << 41) | (1ull << 62)));
  EXPECT(gs::PackVoxel(1, 0, 0) - gs::PackVoxel(0, 0, 0) == 1ull);
  EXPECT(gs::PackVoxel(0, 1, 0) - gs::PackVoxel(0, 0, 0) == (1ull << 21));
  EXPECT(gs::PackVoxel(0, 0, 1) - gs::PackVoxel(0, 0, 0) == (1ull << 42));
  const int edge[] = {-(1 << 20), -(1 << 19), -1, 0, 1, 12345, (1 << 20) - 1};
  for (int x : edge) for (int y : edge) for (int z : edge) {
    int a, b, c;
    gs::UnpackVoxel(gs::PackVoxel(x, y, z), &a, &b, &c);
    EXPECT(a == x && b == y && c == z);
  }
  int a, b, c;
  gs::UnpackVoxel(gs::kNeverVoxel, &a, &b, &c);
  EXPECT(a == -(1 << 20) && a + gs::kMaxHalf < 0);            // no offset of a window lifts it into a box
  gs::Bitmap box; box.extent[0] = 10; box.extent[1] = 4; box.extent[2] = 2;
  EXPECT(gs::Reachable(-3, 0, 0, box, 3, 1) && !gs::Reachable(-4, 0, 0, box, 3, 1) && gs::Reachable(12, 6, 2, box, 3, 1) && !gs::Reachable(13, 0, 0, box, 3, 1));
  EXPECT(!gs::Reachable(0, 7, 0, box, 3, 1) && !gs::Reachable(0, 0, 3, box, 3, 1) && !gs::Reachable(0, 0, -2, box, 3, 1) && gs::Reachable(0, 0, -1, box, 3, 1));
}

static void Sampling() {
  for (long long M : {1LL, 7LL, 4096LL}) {
    for (long long n : {M, M + 1, 2 * M - 1, 3 * M + 2}) {
      EXPECT(gs::SampleCount(n, M) == M);
      long long prev = -1;
      for (long long k = 0; k < M; ++k) {
        const long long r = gs::SampleRow(k, n, M);
        EXPECT(r == (n == M ? k : (k * n) / M) && r > prev && r >= k && r < n);
        prev = r;
      }
    }
    EXPECT(gs::SampleCount(M - 1 > 0 ? M - 1 : 1, M) == (M - 1 > 0 ? M - 1 : 1));
  }
  EXPECT(gs::SampleRow(4095, 2147483647LL, 4096) == (4095LL * 2147483647LL) / 4096);       // 64-bit products
}

static void Yaw() {
  double g[16] = {0.6, 0.8, 0, 0, -0.8, 0.6, 0, 0, 0, 0, 1, 0, 3, -4, 5, 1}, T[12];
  gs::YawTransform(g, 0.0, T);
  EXPECT(T[0] == 0.6 && T[1] == -0.8 && T[3] == 0.8 && T[4] == 0.6 && T[8] == 1 && T[9] == 3 && T[10] == -4 && T[11] == 5);   // a = 0 is the guess itself
  const double ang = 0.3, c = std::cos(ang), s = std::sin(ang);
  gs::YawTransform(g, ang, T);
  EXPECT(T[0] == c * 0.6 - s * 0.8 && T[3] == s * 0.6 + c * 0.8 && T[1] == c * -0.8 - s * 0.6 && T[4] == s * -0.8 + c * 0.6 && T[6] == 0 && T[9] == 3);
}

static void Picking() {
  Args a; a.hxy = 3; a.hz = 1; a.ky = 2;
  gs::Window w;
  EXPECT(Run(a, &w) == gs::kOk);
  for (long long f = 0; f < w.n_candidates; ++f) EXPECT(gs::Encode(gs::Decode(f, w), w) == f);
  { gs::Candidate c; c.a = -2; c.k = -1; c.j = -3; c.i = -3; EXPECT(gs::Encode(c, w) == 0); c.i = -2; EXPECT(gs::Encode(c, w) == 1); c.i = -3; c.j = -2; EXPECT(gs::Encode(c, w) == 7);
    c.j = -3; c.k = 0; EXPECT(gs::Encode(c, w) == 49); c.k = -1; c.a = -1; EXPECT(gs::Encode(c, w) == 147); }
  auto at = [&](int ya, int i, int j, int k) { gs::Candidate c; c.a = ya; c.i = i; c.j = j; c.k = k; return gs::Encode(c, w); };
  std::vector<int32_t> v(static_cast<size_t>(w.n_candidates), 0);
  long long best; int runner;
  auto expect_pick = [&](long long want, int want_runner) { gs::Pick(v.data(), w, &best, &runner); EXPECT(best == want); EXPECT(runner == want_runner); };
  expect_pick(at(0, 0, 0, 0), 0);                                         // all equal: the guess itself
  v[at(1, 2, -1, 0)] = 5;
  expect_pick(at(1, 2, -1, 0), 0);
  v[at(-1, -3, 3, 1)] = 5;                                                // equal score, farther (19 > 5)
  expect_pick(at(1, 2, -1, 0), 5);
  v[at(2, 1, 2, 0)] = 5;                                                  // same distance 5, larger |a|
  expect_pick(at(1, 2, -1, 0), 5);
  v[at(-1, 1, 2, 0)] = 5;                                                 // same distance, same |a|: the smaller a
  expect_pick(at(-1, 1, 2, 0), 5);
  v[at(-1, 0, 2, -1)] = 5;                                                // then the smaller k
  expect_pick(at(-1, 0, 2, -1), 5);
  v[at(-1, 2, 0, -1)] = 5;                                                // then the smaller j
  expect_pick(at(-1, 2, 0, -1), 5);
  v[at(-1, -2, 0, -1)] = 5;                                               // then the smaller i
  expect_pick(at(-1, -2, 0, -1), 5);
  v[at(2, 3, 3, 1)] = 6;                                                  // a higher score beats every tie rule
  expect_pick(at(2, 3, 3, 1), 5);
  // the runner-up: within 2 voxels and 1 yaw step of the pick nothing counts
  std::fill(v.begin(), v.end(), 0);
  v[at(0, 0, 0, 0)] = 9; v[at(0, 2, -2, 1)] = 8; v[at(1, -2, 2, -1)] = 7; v[at(-1, 1, 1, 1)] = 6;
  expect_pick(at(0, 0, 0, 0), 0);
  v[at(0, 3, 0, 0)] = 4; expect_pick(at(0, 0, 0, 0), 4);
  v[at(0, 0, -3, 0)] = 5; expect_pick(at(0, 0, 0, 0), 5);
  v[at(2, 0, 0, 0)] = 6; expect_pick(at(0, 0, 0, 0), 6);
  v[at(-2, 1, 0, 1)] = 7; expect_pick(at(0, 0, 0, 0), 7);
  { gs::Candidate x, y; y.k = 3; EXPECT(gs::Apart(x, y)); y.k = -2; EXPECT(!gs::Apart(x, y)); y.a = -1; EXPECT(!gs::Apart(x, y)); y.a = -2; EXPECT(gs::Apart(x, y)); }
  // one candidate
  Args one; one.hxy = one.hz = one.ky = 0;
  EXPECT(Run(one, &w) == gs::kOk);
  int32_t single = 3;
  gs::Pick(&single, w, &best, &runner);
  EXPECT(best == 0 && runner == 0);
}

// `pick FILE half_xy half_z yaw_steps`: the pick of a volume of int32, printed as "a i j k best_score runner_up_score"
static int PickFile(char** argv) {
  Args a; a.hxy = std::atoi(argv[3]); a.hz = std::atoi(argv[4]); a.ky = std::atoi(argv[5]);
  gs::Window w;
  if (Run(a, &w) != gs::kOk) return 1;
  std::vector<int32_t> v(static_cast<size_t>(w.n_candidates));
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f || std::fread(v.data(), sizeof(int32_t), v.size(), f) != v.size()) return 1;
  std::fclose(f);
  long long best; int runner;
  gs::Pick(v.data(), w, &best, &runner);
  const gs::Candidate c = gs::Decode(best, w);
  std::printf("%d %d %d %d %d %d\n", c.a, c.i, c.j, c.k, v[static_cast<size_t>(best)], runner);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 6 && std::strcmp(argv[1], "pick") == 0) return PickFile(argv);
  Refusals();
  Bitmaps();
  Packing();
  Sampling();
  Yaw();
  Picking();
  if (g_failed) { std::printf("%d checks FAILED\n", g_failed); return 1; }
  std::printf("all checks passed\n");
  return 0;
}
