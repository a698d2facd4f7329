// The host form of the front end's motion compensation (include/smhip/front_end.h) for tests/test_motion_comp_cpp.py.
//   compensate rows.bin delta.bin out.bin   rows: N x 5 float32 (InnerPointType), delta: 16 doubles column-major;
//                                           out.bin: MotionCompensation's N x 5 float32
//   interpolate delta.bin factor            InterpolateTransform(I, delta, factor): 16 numbers, row-major
//   average transforms.bin                  AverageTransforms of K column-major 4x4 doubles: 16 numbers, row-major
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "smhip/front_end.h"

namespace fe = smhip::front_end;
using smhip::data::InnerCloudType;
using smhip::data::InnerPointType;
using smhip::registrator::Matrix4d;

template <typename T>
static std::vector<T> ReadAll(const char* path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
  const std::streamsize bytes = f.tellg();
  f.seekg(0);
  std::vector<T> v(static_cast<size_t>(bytes) / sizeof(T));
  f.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(T)));
  return v;
}

static void Print(const Matrix4d& m) {
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) std::printf("%.17g%s", m(i, j), (i == 3 && j == 3) ? "\n" : " ");
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  if (mode == "compensate" && argc == 5) {
    const std::vector<float> rows = ReadAll<float>(argv[2]);
    const std::vector<double> d = ReadAll<double>(argv[3]);
    if (d.size() != 16 || rows.size() % 5 != 0) return 2;
    InnerCloudType cloud, out;
    cloud.points.resize(rows.size() / 5);
    std::memcpy(static_cast<void*>(cloud.points.data()), rows.data(), rows.size() * sizeof(float));
    Matrix4d delta;
    std::memcpy(delta.data(), d.data(), sizeof(double) * 16);
    fe::MotionCompensation(cloud, delta, &out);
    if (out.points.size() != cloud.points.size()) return 3;
    std::ofstream f(argv[4], std::ios::binary);
    f.write(reinterpret_cast<const char*>(out.points.data()), static_cast<std::streamsize>(out.points.size() * sizeof(InnerPointType)));
    return f.good() ? 0 : 4;
  }
  if (mode == "interpolate" && argc == 4) {
    const std::vector<double> d = ReadAll<double>(argv[2]);
    if (d.size() != 16) return 2;
    Matrix4d delta;
    std::memcpy(delta.data(), d.data(), sizeof(double) * 16);
    Print(fe::InterpolateTransform(Matrix4d::Identity(), delta, static_cast<float>(std::atof(argv[3]))));
    return 0;
  }
  if (mode == "average" && argc == 3) {
    const std::vector<double> d = ReadAll<double>(argv[2]);
    if (d.empty() || d.size() % 16 != 0) return 2;
    std::vector<Matrix4d> transforms(d.size() / 16);
    for (size_t k = 0; k < transforms.size(); ++k) std::memcpy(transforms[k].data(), &d[16 * k], sizeof(double) * 16);
    Print(fe::AverageTransforms(transforms));
    return 0;
  }
  return 2;
}
