// The sequence driver's pose vocabulary (staticmapping_amd/csrc/shard_poses.h), host only, no library:
//   test_shard_poses <dir>      <dir>: a place for the pose files it writes.  Checks the pose chain of the alignment run bit for bit
//                               against the row-major product it used to be computed with, MulPose x AffineInverse, the pose file's
//                               write -> read -> write trip, and where ReadPoses stops.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../staticmapping_amd/csrc/shard_poses.h"

using shard::Pose;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

// row-major 4x4 product: how the driver chained pose_{i+1} = pose_i * T_i before it had MulPose do it
static void Mul4(const double* a, const double* b, double* out) {
  double r[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) { double s = 0; for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j]; r[4 * i + j] = s; }
  std::memcpy(out, r, sizeof(r));
}

static Pose Transposed(const double* m) {
  Pose t{};
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) t[4 * c + r] = m[4 * r + c];
  return t;
}

static uint32_t lcg = 20240607u;
static double U01() { lcg = lcg * 1664525u + 1013904223u; return static_cast<double>(lcg >> 8) / 16777216.0; }

// Rz(a) Ry(b) Rx(c), every angle within 0.2 rad, and a step of at most 1 m; row-major
static void RigidRowMajor(double* m) {
  const double a = 0.4 * U01() - 0.2, b = 0.4 * U01() - 0.2, c = 0.4 * U01() - 0.2;
  const double rz[16] = {std::cos(a), -std::sin(a), 0, 0, std::sin(a), std::cos(a), 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const double ry[16] = {std::cos(b), 0, std::sin(b), 0, 0, 1, 0, 0, -std::sin(b), 0, std::cos(b), 0, 0, 0, 0, 1};
  const double rx[16] = {1, 0, 0, 0, 0, std::cos(c), -std::sin(c), 0, 0, std::sin(c), std::cos(c), 0, 0, 0, 0, 1};
  Mul4(rz, ry, m);
  Mul4(m, rx, m);
  const double d[3] = {2.0 * U01() - 1.0, 2.0 * U01() - 1.0, 2.0 * U01() - 1.0}, len = U01();
  const double norm = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 1e-9;
  for (int r = 0; r < 3; ++r) m[4 * r + 3] = len * d[r] / norm;
}

static double OffIdentity(const Pose& p) {
  double worst = 0.0;
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) worst = std::max(worst, std::fabs(p[4 * c + r] - (r == c ? 1.0 : 0.0)));
  return worst;
}

static std::string Lines(const std::vector<Pose>& poses) {
  std::ostringstream out;
  out.precision(8);                                                       // the pose writer's
  for (const Pose& p : poses) shard::WritePoseLine(out, p.data());
  return out.str();
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: test_shard_poses <dir>\n"); return 2; }
  const std::string dir = argv[1];

  // 1. the chain, once row-major with Mul4 and once column-major with MulPose on the transposed storage: the same doubles
  double row[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  Pose col = Transposed(row);
  std::vector<Pose> chain{col};
  int unequal = 0;
  for (int i = 0; i < 200; ++i) {
    double T[16];
    RigidRowMajor(T);
    const Pose Tc = Transposed(T);
    Mul4(row, T, row);
    col = shard::MulPose(col, Tc);
    const Pose want = Transposed(row);
    if (std::memcmp(want.data(), col.data(), sizeof(double) * 16) != 0) ++unequal;
    chain.push_back(col);
    EXPECT(OffIdentity(shard::MulPose(Tc, shard::AffineInverse(Tc))) < 1e-12);
    EXPECT(OffIdentity(shard::MulPose(col, shard::AffineInverse(col))) < 1e-12);
  }
  EXPECT(unequal == 0);
  EXPECT(std::fabs(col[12]) + std::fabs(col[13]) + std::fabs(col[14]) > 1.0);   // (the chain went somewhere)

  // 2. write -> read -> write gives the same bytes, and a line's 12 numbers land at m[4 * c + r] with m[15] == 1
  const std::string text = Lines(chain);
  { std::ofstream f(dir + "/chain.txt"); f << text; }
  std::vector<Pose> back;
  EXPECT(shard::ReadPoses(dir + "/chain.txt", &back));
  EXPECT(back.size() == chain.size());
  EXPECT(Lines(back) == text);
  EXPECT(text.compare(0, 24, "1 0 0 0 0 1 0 0 0 0 1 0\n") == 0);          // a space between two numbers, none at either end
  { std::ofstream f(dir + "/counted.txt"); f << "1 2 3 4 5 6 7 8 9 10 11 12\n"; }
  std::vector<Pose> counted;
  EXPECT(shard::ReadPoses(dir + "/counted.txt", &counted) && counted.size() == 1);
  if (counted.size() == 1) {
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) EXPECT(counted[0][4 * c + r] == 4 * r + c + 1);
    EXPECT(counted[0][3] == 0.0 && counted[0][7] == 0.0 && counted[0][11] == 0.0 && counted[0][15] == 1.0);
  }

  // 3. reading stops at the first line with fewer than twelve numbers and keeps the lines before it; no file: false
  { std::ofstream f(dir + "/short.txt"); f << Lines({chain[1], chain[2], chain[3]}) << "1 0 0 0 0 1 0 0 0 0 1\n" << Lines({chain[4]}); }
  std::vector<Pose> kept;
  EXPECT(shard::ReadPoses(dir + "/short.txt", &kept));
  EXPECT(kept.size() == 3 && Lines(kept) == Lines({chain[1], chain[2], chain[3]}));
  std::vector<Pose> none;
  EXPECT(!shard::ReadPoses(dir + "/no_such_file.txt", &none) && none.empty());

  if (failures == 0) std::printf("all checks passed\n");
  return failures == 0 ? 0 : 1;
}
