// Time of the header's host MotionCompensation (include/smhip/front_end.h) on one scan, for tools/motion_comp_probe.py.
// argv: rows.bin (N x 5 float32) delta.bin (16 doubles, column-major) repeats warmup -> one JSON line with the median ms
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "smhip/front_end.h"

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  std::ifstream f(argv[1], std::ios::binary | std::ios::ate);
  if (!f) return 2;
  const size_t n = static_cast<size_t>(f.tellg()) / (5 * sizeof(float));
  f.seekg(0);
  smhip::data::InnerCloudType cloud, out;
  cloud.points.resize(n);
  f.read(reinterpret_cast<char*>(cloud.points.data()), static_cast<std::streamsize>(n * 5 * sizeof(float)));
  smhip::registrator::Matrix4d delta;
  std::ifstream g(argv[2], std::ios::binary);
  if (!g.read(reinterpret_cast<char*>(delta.data()), sizeof(double) * 16)) return 2;
  const int repeats = std::atoi(argv[3]), warmup = std::atoi(argv[4]);
  std::vector<double> ms;
  double checksum = 0;
  for (int r = 0; r < warmup + repeats; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    smhip::front_end::MotionCompensation(cloud, delta, &out);
    const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    checksum += out.points[out.points.size() / 2].x;
    if (r >= warmup) ms.push_back(t);
  }
  std::sort(ms.begin(), ms.end());
  std::printf("{\"points\": %zu, \"repeats\": %d, \"median_ms\": %.4f, \"checksum\": %.9g}\n", n, repeats, ms[ms.size() / 2], checksum);
  return 0;
}
