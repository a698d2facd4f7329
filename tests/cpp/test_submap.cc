// static_map::Submap's bookkeeping and the matching of consecutive submaps (include/smhip/submap.h).
//   test_submap host                                  no device: local poses, Full(), the refused insert, the voxel size's trip
//                                                     through the filter text, the order of ConsecutivePairs
//   test_submap match <dir> <scans> <frame_count> <points per scan> <voxel_size>
//                                                     <dir>/NNNNNN.bin KITTI scans and <dir>/poses.txt (16 doubles per line, row-major
//                                                     4x4 global pose per scan): submaps of frame_count scans through ConnectSubmaps
//                                                     (IcpFast) and, for the first pair, the device forms ToSource / ToTarget; one JSON line
#define SMHIP_REGISTRATOR_THROW_ON_CHECK 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "smhip/submap.h"

namespace reg = smhip::registrator;
namespace bld = smhip::builder;
using smhip::data::InnerCloudType;
using smhip::data::InnerPointType;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static reg::Matrix4d Pose(double x, double y, double yaw_deg) {
  reg::Matrix4d p = reg::Matrix4d::Identity();
  const double a = yaw_deg * M_PI / 180.0;
  p(0, 0) = std::cos(a); p(0, 1) = -std::sin(a); p(1, 0) = std::sin(a); p(1, 1) = std::cos(a);
  p(0, 3) = x; p(1, 3) = y;
  return p;
}
static double MaxDiff(const reg::Matrix4d& a, const reg::Matrix4d& b) {
  double d = 0;
  for (int q = 0; q < 16; ++q) d = std::max(d, std::fabs(a.data()[q] - b.data()[q]));
  return d;
}
static InnerCloudType::Ptr SmallCloud(int n) {
  InnerCloudType::Ptr c(new InnerCloudType);
  c->points.resize(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) { c->points[i].x = 0.1f * i; c->points[i].y = 1.f; c->points[i].z = -0.5f; }
  return c;
}

static int HostChecks() {
  bld::SubmapOptions defaults;
  EXPECT(defaults.frame_count == 5 && !defaults.enable_voxel_filter && defaults.voxel_size == 0.1f);   // submap_options.h:30-38
  bld::SubmapOptions opt;
  opt.frame_count = 3; opt.enable_voxel_filter = true; opt.voxel_size = 0.1234567f;
  const reg::Matrix4d poses[4] = {Pose(1.0, 0.0, 0.0), Pose(1.8, 0.1, 5.0), Pose(2.6, 0.2, 10.0), Pose(3.4, 0.3, 15.0)};
  bld::Submap s(opt);
  for (int k = 0; k < 3; ++k) {
    EXPECT(!s.Full() && s.FrameCount() == k);
    s.InsertFrame(SmallCloud(10 + k), poses[k]);
  }
  EXPECT(s.Full() && s.FrameCount() == 3 && s.TotalPoints() == 33);
  bool refused = false;
  try { s.InsertFrame(SmallCloud(4), poses[3]); } catch (const std::runtime_error&) { refused = true; }   // CHECK(!full_), submap.cc:78
  EXPECT(refused && s.FrameCount() == 3);
  EXPECT(MaxDiff(s.LocalPose(0), reg::Matrix4d::Identity()) == 0.0);
  EXPECT(MaxDiff(s.FirstFramePose(), poses[0]) == 0.0);
  for (int k = 1; k < 3; ++k) {
    // local pose = submap pose^-1 * frame pose (:87): back on the frame pose when the submap pose is applied again
    EXPECT(MaxDiff(smhip::back_end::Multiply(poses[0], s.LocalPose(k)), poses[k]) < 1e-15);
    const double yaw = std::atan2(s.LocalPose(k)(1, 0), s.LocalPose(k)(0, 0)) * 180.0 / M_PI;
    EXPECT(std::fabs(yaw - 5.0 * k) < 1e-12 && std::fabs(s.LocalPose(k)(0, 3) - 0.8 * k) < 1e-12 && std::fabs(s.LocalPose(k)(1, 3) - 0.1 * k) < 1e-12);
  }
  // the voxel size as the filter text carries it: six decimals, then float
  EXPECT(s.DeviceVoxelSize() == 0.123457f);
  EXPECT(bld::TextVoxelSize(0.1f) == 0.1f && bld::TextVoxelSize(0.1234564f) == 0.123456f);
  EXPECT(bld::Submap(defaults).DeviceVoxelSize() == 0.f);                                              // enable_voxel_filter = false
  // ConsecutivePairs: source = the later submap, target = the earlier one (map_builder.cc:399-404), guess = target^-1 * source
  // (:426-428); the trailing submap that is not full takes part in no pair
  std::vector<std::shared_ptr<bld::Submap>> maps;
  for (int m = 0; m < 4; ++m) {
    maps.emplace_back(new bld::Submap(opt));
    for (int k = 0; k < (m < 3 ? 3 : 2); ++k) maps.back()->InsertFrame(SmallCloud(5), Pose(2.4 * m + 0.8 * k, 0.3 * m, 4.0 * m + k));
  }
  const auto pairs = bld::ConsecutivePairs(maps);
  EXPECT(pairs.size() == 2);
  for (size_t k = 0; k < pairs.size(); ++k) {
    EXPECT(pairs[k].source == static_cast<int>(k) + 1 && pairs[k].target == static_cast<int>(k));
    const reg::Matrix4d back = smhip::back_end::Multiply(maps[k]->FirstFramePose(), pairs[k].guess);
    EXPECT(MaxDiff(back, maps[k + 1]->FirstFramePose()) < 1e-14);
    EXPECT(std::fabs(pairs[k].guess(0, 3)) > 1.0);                                                     // not the inverse direction's zero
  }
  // target^-1 * source, not source^-1 * target: the guess moves source coordinates into the target's frame
  EXPECT(pairs[0].guess(0, 3) > 0.0);
  std::printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}

static InnerCloudType::Ptr ReadKittiBin(const std::string& path) {      // ros_node/kitti_reader.cc:91-121, factor as data_collector.h:202-204
  std::ifstream f(path, std::ios::binary);
  InnerCloudType::Ptr c(new InnerCloudType);
  float row[4];
  while (f.read(reinterpret_cast<char*>(row), sizeof(row))) { InnerPointType p; p.x = row[0]; p.y = row[1]; p.z = row[2]; p.intensity = row[3]; c->points.push_back(p); }
  for (size_t i = 0; i < c->points.size(); ++i) c->points[i].factor = static_cast<float>(static_cast<double>(i) / c->points.size());
  return c;
}
static void PrintMatrix(const char* key, const reg::Matrix4d& m) {
  std::printf("\"%s\": [", key);
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) std::printf("%.17g%s", m(r, c), (r == 3 && c == 3) ? "" : ", ");
  std::printf("], ");
}

static int Match(int argc, char** argv) {
  if (argc < 7) return 2;
  const std::string dir = argv[2];
  const int scans = std::atoi(argv[3]), frame_count = std::atoi(argv[4]), points = std::atoi(argv[5]);
  bld::SubmapOptions opt;
  opt.frame_count = frame_count; opt.enable_voxel_filter = std::atof(argv[6]) > 0; opt.voxel_size = static_cast<float>(std::atof(argv[6]));
  std::ifstream pf(dir + "/poses.txt");
  std::vector<std::shared_ptr<bld::Submap>> maps;
  for (int k = 0; k < scans; ++k) {
    reg::Matrix4d P;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) pf >> P(r, c);
    if (maps.empty() || maps.back()->Full()) maps.emplace_back(new bld::Submap(opt));
    char name[32];
    std::snprintf(name, sizeof(name), "/%06d.bin", k);
    maps.back()->InsertFrame(ReadKittiBin(dir + name), P);
  }
  auto context = std::make_shared<bld::DeviceContext>(0, frame_count * points);
  reg::MatcherOptions mopt;
  mopt.type = reg::kFastIcp;
  mopt.accepted_min_score = 0.7f;
  auto matcher = reg::CreateMatcher(mopt, false);
  const auto results = bld::ConnectSubmaps(mopt, matcher, maps, context);
  std::printf("{\"pairs\": %zu, ", results.size());
  for (size_t k = 0; k < results.size(); ++k) {
    const std::string i = std::to_string(k);
    PrintMatrix(("transform" + i).c_str(), results[k].transform_to_next);
    PrintMatrix(("guess" + i).c_str(), results[k].guess);
    std::printf("\"score%s\": %.17g, \"accepted%s\": %s, ", i.c_str(), results[k].match_score, i.c_str(), results[k].accepted ? "true" : "false");
  }
  // the device forms on a matcher of their own: submap 1 as source on submap 0 as target, no download
  reg::IcpFastHip device_matcher(0, 4096);
  device_matcher.InitWithOptions();
  const int nt = maps[0]->ToTarget(&device_matcher);
  const int ns = maps[1]->ToSource(&device_matcher);
  reg::Matrix4d resident = reg::Matrix4d::Identity();
  const bool ok = device_matcher.Align(results[0].guess, resident);
  PrintMatrix("resident_transform", resident);
  std::printf("\"resident_ok\": %s, \"resident_score\": %.17g, \"resident_ns\": %d, \"resident_nt\": %d, \"cloud0\": %d, \"cloud1\": %d}\n",
              ok ? "true" : "false", device_matcher.GetFitnessScore(), ns, nt, static_cast<int>(maps[0]->Cloud()->GetInnerCloud().size()),
              static_cast<int>(maps[1]->Cloud()->GetInnerCloud().size()));
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "host") return HostChecks();
  if (argc >= 2 && std::string(argv[1]) == "match") return Match(argc, argv);
  std::fprintf(stderr, "usage: test_submap host | match <dir> <scans> <frame_count> <points per scan> <voxel_size>\n");
  return 2;
}
