// MapBuilder::ScanMatchProcessing with motion compensation (include/smhip/front_end.h) over a short synthetic drive.
// argv: n_scans dir vx vy device_target_prep enable use_average [out_dir]
//   dir holds 0000000000.bin ... (KITTI rows; factor = i / n as the collector sets it).  Prints one JSON line: per frame the key and
//   matched flags, the score, the wall time, and -- row-major 4x4, 17 digits -- the pose, the guess, the matcher's raw result, both
//   deltas and the averaged transform.  With out_dir, the cloud ProcessCloud leaves in the caller's hands (the second pass's rows
//   when compensation is enabled) is written to out_dir/frame_<k>.bin as N x 5 float32.
// With enable = 0 the "key", "matched", "score", "ms" and "pose" entries are what tests/cpp/test_front_end.cc prints.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "smhip/front_end.h"

namespace reg = smhip::registrator;
using smhip::data::InnerPointCloudData;
using smhip::data::InnerPointType;

static std::vector<InnerPointType> ReadKittiBin(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<InnerPointType> pts;
  float row[4];
  while (f.read(reinterpret_cast<char*>(row), sizeof(row))) { InnerPointType p; p.x = row[0]; p.y = row[1]; p.z = row[2]; p.intensity = row[3]; pts.push_back(p); }
  for (size_t i = 0; i < pts.size(); ++i) pts[i].factor = static_cast<float>(static_cast<double>(i) / pts.size());
  return pts;
}

static void PrintMatrix(const char* name, const reg::Matrix4d& m, const char* tail) {
  std::printf("\"%s\": [", name);
  for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) std::printf("%.17g%s", m(i, j), (i == 3 && j == 3) ? "" : ", ");
  std::printf("]%s", tail);
}

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const int n = std::atoi(argv[1]);
  reg::MatcherOptions opt;
  opt.type = reg::kFastIcp;                                        // config/lidar_only.xml:46
  opt.registrator_options_node = "<param name=\"max_iteration\"> 100 </param><param name=\"dist_outlier_ratio\"> 0.7 </param>";
  auto matcher = reg::CreateMatcher(opt);
  if (!matcher) return 3;
  smhip::front_end::MotionFilter mf;
  mf.translation_range = 0.5f;
  const bool device_prep = std::atoi(argv[5]) != 0;
  smhip::front_end::MotionCompensationOptions mc;                  // config/lidar_only.xml:75-77
  mc.enable = std::atoi(argv[6]) != 0;
  mc.use_average = std::atoi(argv[7]) != 0;
  smhip::front_end::ScanMatcherFrontEnd fe(matcher, mf, true, device_prep, mc);
  if (device_prep && !fe.DeviceTargetPrep()) return 4;
  fe.Extrapolator().InitRoughLinearVelocity(std::atof(argv[3]), std::atof(argv[4]), 0.0);   // pose_extrapolator.cc:210-214
  const std::string out_dir = argc > 8 ? argv[8] : "";
  std::printf("{\"frames\": [");
  for (int k = 0; k < n; ++k) {
    char name[64];
    std::snprintf(name, sizeof(name), "/%010d.bin", k);
    InnerPointCloudData::Ptr cloud(new InnerPointCloudData(ReadKittiBin(std::string(argv[2]) + name)));
    const auto t0 = std::chrono::steady_clock::now();
    const auto r = fe.ProcessCloud(cloud, 0.1 * k);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%s{\"key\": %s, \"matched\": %s, \"score\": %.9g, \"ms\": %.3f, ", k ? ", " : "", r.new_key_frame ? "true" : "false",
                r.matched ? "true" : "false", r.score, ms);
    PrintMatrix("pose", r.pose, ", ");
    PrintMatrix("guess", r.guess, ", ");
    PrintMatrix("raw_result", r.raw_result, ", ");
    PrintMatrix("first_delta", r.first_delta, ", ");
    PrintMatrix("second_delta", r.second_delta, ", ");
    PrintMatrix("average", r.average_transform, "}");
    if (!out_dir.empty()) {
      std::snprintf(name, sizeof(name), "/frame_%d.bin", k);
      std::ofstream f(out_dir + name, std::ios::binary);
      const auto& rows = cloud->GetInnerCloud();
      f.write(reinterpret_cast<const char*>(rows.data()), static_cast<std::streamsize>(rows.size() * sizeof(InnerPointType)));
      if (!f.good()) return 5;
    }
  }
  std::printf("]}\n");
  return 0;
}
