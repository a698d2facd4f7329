// shard_poses.h -- the sequence driver's poses: column-major 4x4 doubles, their product and inverse, and the pose file's lines.
// Host-only C++ with no HIP and no library behind it (tests/cpp/test_shard_poses.cc compiles it alone).
#pragma once

#include <array>
#include <cstdlib>
#include <fstream>
#include <ostream>
#include <string>
#include <vector>

namespace shard {

using Pose = std::array<double, 16>;                                      // column-major: m[4 * c + r]

inline Pose MulPose(const Pose& a, const Pose& b) {                       // a * b
  Pose out{};
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) { double s = 0; for (int k = 0; k < 4; ++k) s += a[4 * k + r] * b[4 * c + k]; out[4 * c + r] = s; }
  return out;
}

// inverse of an affine 4x4, what Eigen's inverse() gives for a pose: the 3x3 block by its adjugate
inline Pose AffineInverse(const Pose& p) {
  auto m = [&](int r, int c) { return p[4 * c + r]; };
  const double c00 = m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1), c01 = m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2), c02 = m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0);
  const double det = m(0, 0) * c00 + m(0, 1) * c01 + m(0, 2) * c02;
  double inv[3][3] = {{c00 / det, (m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2)) / det, (m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1)) / det},
                      {c01 / det, (m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0)) / det, (m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2)) / det},
                      {c02 / det, (m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1)) / det, (m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)) / det}};
  Pose out{};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out[4 * c + r] = inv[r][c];
    out[12 + r] = -(inv[r][0] * m(0, 3) + inv[r][1] * m(1, 3) + inv[r][2] * m(2, 3));
  }
  out[15] = 1.0;
  return out;
}

// kitti_pose.txt (map_builder.cc:626-641): 12 numbers per line, the row-major top 3x4 -> column-major 4x4.  Reading stops at the
// first line that does not hold 12 numbers.  false: the file cannot be opened.
inline bool ReadPoses(const std::string& path, std::vector<Pose>* poses) {
  std::ifstream f(path);
  if (!f) return false;
  std::string text;
  while (std::getline(f, text)) {
    double v[12];
    const char* p = text.c_str();
    int got = 0;
    for (; got < 12; ++got) {
      char* end = nullptr;
      v[got] = std::strtod(p, &end);
      if (end == p) break;
      p = end;
    }
    if (got < 12) break;
    Pose m{};
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m[4 * c + r] = v[4 * r + c];
    m[15] = 1.0;
    poses->push_back(m);
  }
  return true;
}

// one line of that file: the top 3 x 4 row by row, a space between two numbers, at the stream's precision (the pose writer's is 8)
inline void WritePoseLine(std::ostream& out, const double* column_major) {
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) out << column_major[4 * c + r] << ((r == 2 && c == 3) ? "\n" : " ");
}

}  // namespace shard
