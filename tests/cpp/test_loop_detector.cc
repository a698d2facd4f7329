// back_end::LoopDetector (include/smhip/back_end.h), the restatement of the reference's back_end/loop_detector.cc.
//   test_loop_detector host                           no device: candidate selection, the loop machine, CheckResult
//   test_loop_detector gpu <dir> <scans> <frame_count> <m2dp_match_score>
//                                                     <dir>/NNNNNN.bin KITTI scans and <dir>/poses.txt (16 doubles per line, row-major
//                                                     4x4 global pose per scan): submaps of frame_count scans at voxel 0.1, their
//                                                     device descriptors, the detector over them, and CloseLoop called directly on
//                                                     the pairs it chose; one JSON line
#define SMHIP_REGISTRATOR_THROW_ON_CHECK 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "smhip/submap.h"

namespace reg = smhip::registrator;
namespace bld = smhip::builder;
namespace be = smhip::back_end;
using smhip::data::InnerCloudType;
using smhip::data::InnerPointType;
using Descriptor = smhip::descriptor::M2dp::Descriptor;
using Pairs = std::vector<std::pair<int, int>>;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static reg::Matrix4d Pose(double x, double y, double z, double yaw) {
  reg::Matrix4d p = reg::Matrix4d::Identity();
  p(0, 0) = std::cos(yaw); p(0, 1) = -std::sin(yaw); p(1, 0) = std::sin(yaw); p(1, 1) = std::cos(yaw);
  p(0, 3) = x; p(1, 3) = y; p(2, 3) = z;
  return p;
}

// n frames, the newest (current) at the origin, every other one far away (100 m) unless placed
struct Track {
  std::vector<std::array<double, 3>> t;
  std::vector<Descriptor> d;
  explicit Track(int n) : t(static_cast<size_t>(n), std::array<double, 3>{100.0, 0.0, 0.0}), d(static_cast<size_t>(n), Ramp(1.0)) { t.back() = {0.0, 0.0, 0.0}; }
  static Descriptor Ramp(double sign) {            // 16 values: squares for Ramp(1), alternating 1 and 9 for Ramp(-1); their score is far below 0.99
    Descriptor v(16);
    for (int i = 0; i < 16; ++i) v[static_cast<size_t>(i)] = sign > 0 ? static_cast<float>(i * i) + 1.f : (i % 2 ? 9.f : 1.f);
    return v;
  }
  be::LoopCandidates Select(const be::LoopDetectorSettings& s, int w0 = -1, int w1 = -1) const {
    std::vector<const Descriptor*> p;
    for (const auto& v : d) p.push_back(&v);
    return be::SelectLoopCandidates(s, t, p, w0, w1);
  }
};
static Pairs With(const std::vector<int>& targets, int current) {
  Pairs p;
  for (int i : targets) p.emplace_back(i, current);
  return p;
}

static void CandidateChecks() {
  be::LoopDetectorSettings def;                                                  // loop_detector_options.h:29-40
  EXPECT(!def.use_gps && !def.use_descriptor && !def.output_matched_cloud && def.loop_ignore_threshold == 15 && def.trying_detect_loop_count == 1 &&
         def.nearest_history_pos_num == 4 && def.max_close_loop_distance == 25.f && def.max_close_loop_z_distance == 1.f &&
         def.m2dp_match_score == 0.99f && def.accept_scan_match_score == 0.75f);
  be::LoopDetectorSettings s;
  s.loop_ignore_threshold = 3;
  {   // the ignore threshold bounds the search: end_index = max_index - threshold (:80)
    Track k(10);
    for (int i = 0; i < 9; ++i) k.t[static_cast<size_t>(i)] = {12.0 + i, 0.0, 0.0};           // all within 25 m, none within 10 m
    const auto c = k.Select(s);
    EXPECT(c.indices_in_distance == std::vector<int>({0, 1, 2, 3, 4, 5}) && c.closest_index == -1 && c.loop_detection == 1);
    // the window replaces both ends and is clamped to the newest index (:81-84): frames inside the threshold are searched too
    EXPECT(k.Select(s, 2, 100).indices_in_distance == std::vector<int>({2, 3, 4, 5, 6, 7, 8}));
    EXPECT(k.Select(s, 4, 6).indices_in_distance == std::vector<int>({4, 5}));
    EXPECT(k.Select(s, 0, 0).indices_in_distance.empty() && k.Select(s, 0, 0).loop_detection == 0);
    EXPECT(k.Select(s, -1, 5).indices_in_distance.size() == 6);                                // a negative end of the window: no window
  }
  {   // the z gate (<=) and the xy gate (<=)
    Track k(8);
    k.t[0] = {25.0, 0.0, 1.0}; k.t[1] = {15.0, 20.0, -1.0}; k.t[2] = {3.0, 0.0, 1.5}; k.t[3] = {25.1, 0.0, 0.0}; k.t[4] = {3.0, 0.0, 0.0};
    const auto c = k.Select(s);                                                                // searched: 0..3 (7 - 3 = 4)
    EXPECT(c.indices_in_distance == std::vector<int>({0, 1}) && c.closest_index == -1);
  }
  {   // the 0.4 rule: the closest index is dropped at min_distance >= 10 (:98-100)
    Track k(8);
    k.t[1] = {0.0, 9.99, 0.0}; k.t[2] = {12.0, 0.0, 0.0};
    EXPECT(k.Select(s).closest_index == 1);
    k.t[1] = {0.0, 10.0, 0.0};
    EXPECT(k.Select(s).closest_index == -1 && k.Select(s).indices_in_distance == std::vector<int>({1, 2}));
    k.t[1] = {6.0, 8.0, 0.0};                                                                  // norm exactly 10
    EXPECT(k.Select(s).closest_index == -1);
  }
  {   // the step rule with nearest_history_pos_num = 4 (:129-145) and the closest pair (:146-152)
    s.loop_ignore_threshold = 1;
    auto track = [](int well, int closest) {
      Track k(well + 2);
      for (int i = 0; i < well; ++i) k.t[static_cast<size_t>(i)] = {12.0 + 0.5 * i, 0.0, 0.0};
      if (closest >= 0) k.t[static_cast<size_t>(closest)] = {0.0, 5.0, 0.0};
      return k;
    };
    EXPECT(track(3, -1).Select(s).maybe_close_pair == With({0, 1, 2}, 4));                     // fewer than 4: all of them
    EXPECT(track(5, -1).Select(s).maybe_close_pair == With({0, 1, 2, 3}, 6));                  // 4 < size < 8: the first 4
    EXPECT(track(8, -1).Select(s).maybe_close_pair == With({0, 2, 4, 6}, 9));                  // size >= 8: step = 8 / 4 = 2
    EXPECT(track(9, -1).Select(s).maybe_close_pair == With({0, 2, 4, 6}, 10));                 // step = 9 / 4 = 2
    EXPECT(track(12, -1).Select(s).maybe_close_pair == With({0, 3, 6, 9}, 13));
    EXPECT(track(9, 7).Select(s).maybe_close_pair == With({0, 2, 4, 6, 7}, 10));               // the closest pair is appended
    EXPECT(track(9, 4).Select(s).maybe_close_pair == With({0, 2, 4, 6}, 10));                  // ... but not twice
    EXPECT(track(3, 1).Select(s).maybe_close_pair == With({0, 1, 2}, 4));
    EXPECT(track(5, 4).Select(s).maybe_close_pair == With({0, 1, 2, 3, 4}, 6));
  }
  {   // the descriptor gate: on, only frames whose score is ABOVE m2dp_match_score; off, a copy of the distance gate
    s.loop_ignore_threshold = 1;
    Track k(7);
    for (int i = 0; i < 5; ++i) k.t[static_cast<size_t>(i)] = {12.0 + i, 0.0, 0.0};
    k.t[3] = {0.0, 5.0, 0.0};
    k.d[1] = Track::Ramp(-1.0); k.d[3] = Track::Ramp(-1.0);
    const double low = smhip::descriptor::matchTwoM2dpDescriptors(k.d[6], k.d[1]), same = smhip::descriptor::matchTwoM2dpDescriptors(k.d[6], k.d[0]);
    EXPECT(low >= 0.0 && low < 0.9 && std::fabs(same - 1.0) < 1e-12);
    EXPECT(k.Select(s).indices_well_matched == std::vector<int>({0, 1, 2, 3, 4}));
    s.use_descriptor = true;
    auto c = k.Select(s);
    EXPECT(c.indices_well_matched == std::vector<int>({0, 2, 4}) && c.closest_index == 3);
    EXPECT(c.maybe_close_pair == With({0, 2, 4, 3}, 6));                                        // the closest pair needs no descriptor match
    for (auto& v : k.d) v = Track::Ramp(-1.0);
    k.d[6] = Track::Ramp(1.0);
    c = k.Select(s);
    EXPECT(c.loop_detection == 0 && c.maybe_close_pair.empty() && c.indices_in_distance.size() == 5);   // ... unless nothing matched at all
    s.m2dp_match_score = static_cast<float>(low) - 0.01f;
    EXPECT(k.Select(s).indices_well_matched.size() == 5);
    s.m2dp_match_score = 1.0f;                                                                 // the score must be above, not equal
    for (auto& v : k.d) v = Track::Ramp(1.0);
    const double one = smhip::descriptor::matchTwoM2dpDescriptors(k.d[6], k.d[0]);
    EXPECT((one > 1.0f) == !k.Select(s).indices_well_matched.empty());
    EXPECT(smhip::descriptor::matchTwoM2dpDescriptors(k.d[0], Descriptor(15, 1.f)) == -1.0);
    EXPECT(smhip::descriptor::matchTwoM2dpDescriptors(Descriptor(9, 1.f), Descriptor(9, 2.f)) == -1.0);
  }
}

static void MachineChecks() {
  using S = be::LoopStatus;
  be::LoopDetectorSettings one, two;
  two.trying_detect_loop_count = 2;
  int n = 7;
  EXPECT(be::NextLoopStatus(S::kNoLoop, 0, one, &n) == S::kNoLoop && n == 0);
  EXPECT(be::NextLoopStatus(S::kNoLoop, 1, one, &n) == S::kEnteringLoop && n == 1);
  n = 7;
  EXPECT(be::NextLoopStatus(S::kNoLoop, 1, two, &n) == S::kTryingToCloseLoop && n == 1);
  EXPECT(be::NextLoopStatus(S::kTryingToCloseLoop, 1, two, &n) == S::kEnteringLoop && n == 2);
  n = 0;
  EXPECT(be::NextLoopStatus(S::kTryingToCloseLoop, 0, two, &n) == S::kNoLoop);
  be::LoopDetectorSettings three;
  three.trying_detect_loop_count = 3;
  n = 1;
  EXPECT(be::NextLoopStatus(S::kTryingToCloseLoop, 1, three, &n) == S::kTryingToCloseLoop && n == 2);
  EXPECT(be::NextLoopStatus(S::kEnteringLoop, 0, one, &n) == S::kTryingToCloseLoop);
  EXPECT(be::NextLoopStatus(S::kEnteringLoop, 1, one, &n) == S::kContinousLoop);
  n = 5;
  EXPECT(be::NextLoopStatus(S::kContinousLoop, 1, one, &n) == S::kContinousLoop && n == 5);
  EXPECT(be::NextLoopStatus(S::kContinousLoop, 0, one, &n) == S::kLeavingLoop && n == 0);
  EXPECT(be::NextLoopStatus(S::kLeavingLoop, 0, one, &n) == S::kNoLoop);
  EXPECT(be::NextLoopStatus(S::kLeavingLoop, 1, one, &n) == S::kTryingToCloseLoop);

  // through AddFrame: frames without clouds, so the machine runs up to kEnteringLoop; kContinousLoop needs the clouds
  be::LoopDetectorSettings s;
  s.loop_ignore_threshold = 2;
  be::LoopDetector det(s);
  std::vector<std::shared_ptr<be::LoopFrame>> f;
  const double xs[6] = {0.0, 3.0, 60.0, 90.0, 1.0, 2.0};
  for (int k = 0; k < 6; ++k) { f.emplace_back(new be::LoopFrame); f.back()->global_pose = Pose(xs[k], 0.0, 0.0, 0.0); }
  for (int k = 0; k < 3; ++k) {                                                                // size <= threshold: nothing is searched
    const be::DetectResult r = det.AddFrame(f[static_cast<size_t>(k)]);
    EXPECT(r.status == S::kNoLoop && r.current_frame_index == k && r.edges.empty() && det.Status() == S::kNoLoop);
  }
  be::DetectResult r = det.AddFrame(f[3]);                                                    // frame 0 is 90 m away
  EXPECT(det.Status() == S::kNoLoop && det.LastCandidates().loop_detection == 0);
  r = det.AddFrame(f[4], false);                                                               // do_loop_detect = false: the frame is kept, no search
  EXPECT(det.Status() == S::kNoLoop && r.current_frame_index == 4 && det.GetFrames().size() == 5);
  // the positions are read again on every call: frame 2 moves next to the coming frame
  f[2]->global_pose = Pose(2.5, 0.0, 0.0, 0.0);
  r = det.AddFrame(f[5]);
  EXPECT(r.status == S::kNoLoop && det.Status() == S::kEnteringLoop);                          // the result carries the status before the frame (:62)
  EXPECT(det.LastCandidates().maybe_close_pair == With({0, 1, 2}, 5) && det.LastCandidates().closest_index == 2);
  bool refused = false;
  std::shared_ptr<be::LoopFrame> g(new be::LoopFrame);
  g->global_pose = Pose(2.0, 0.5, 0.0, 0.0);
  try { det.AddFrame(g); } catch (const std::runtime_error&) { refused = true; }               // kContinousLoop without clouds
  EXPECT(refused && det.Status() == S::kContinousLoop);
  bool bad_window = false;
  try { det.SetSearchWindow(3, 2); } catch (const std::runtime_error&) { bad_window = true; }
  EXPECT(bad_window);
  det.SetSearchWindow(1, 2);
}

static void CheckResultChecks() {
  // every edge says where the source is: target pose * transform; they must agree within 0.25 m and 0.02 rad (:339)
  const reg::Matrix4d source = Pose(5.0, 1.0, 0.2, 0.3);
  const reg::Matrix4d targets[3] = {Pose(0.0, 0.0, 0.0, 0.0), Pose(2.0, -1.0, 0.1, 0.1), Pose(4.0, 3.0, 0.0, -0.2)};
  auto edges_for = [&](double dx, double dyaw, int n) {
    std::vector<be::LoopEdge> e(static_cast<size_t>(n));
    for (int k = 0; k < n; ++k) {
      reg::Matrix4d want = source;
      if (k == n - 1) want = be::Multiply(source, Pose(dx, 0.0, 0.0, dyaw));                 // the last edge disagrees by (dx, dyaw)
      e[static_cast<size_t>(k)].transform = be::Multiply(be::RigidInverse(targets[k]), want);
      e[static_cast<size_t>(k)].close_pair_index = {k, 9};
    }
    return e;
  };
  const std::vector<reg::Matrix4d> poses(targets, targets + 3);
  EXPECT(!be::CheckLoopResult(edges_for(0.0, 0.0, 1), poses));                                 // one edge is never enough (:321-323)
  EXPECT(be::CheckLoopResult(edges_for(0.0, 0.0, 2), poses) && be::CheckLoopResult(edges_for(0.0, 0.0, 3), poses));
  EXPECT(be::CheckLoopResult(edges_for(0.24, 0.0, 3), poses) && !be::CheckLoopResult(edges_for(0.26, 0.0, 3), poses));
  EXPECT(be::CheckLoopResult(edges_for(0.0, 0.019, 3), poses) && !be::CheckLoopResult(edges_for(0.0, 0.021, 3), poses));
  EXPECT(be::CheckLoopResult(edges_for(0.0, -0.019, 2), poses) && !be::CheckLoopResult(edges_for(0.0, -0.021, 2), poses));
  double e[3];
  be::RotationMatrixToEulerAngles(Pose(0, 0, 0, 0.4), e);
  EXPECT(e[0] == 0.0 && e[1] == 0.0 && std::fabs(e[2] - 0.4) < 1e-15);
}

static InnerCloudType::Ptr ReadKittiBin(const std::string& path) {      // ros_node/kitti_reader.cc:91-121, factor as data_collector.h:202-204
  std::ifstream f(path, std::ios::binary);
  InnerCloudType::Ptr c(new InnerCloudType);
  float row[4];
  while (f.read(reinterpret_cast<char*>(row), sizeof(row))) { InnerPointType p; p.x = row[0]; p.y = row[1]; p.z = row[2]; p.intensity = row[3]; c->points.push_back(p); }
  for (size_t i = 0; i < c->points.size(); ++i) c->points[i].factor = static_cast<float>(static_cast<double>(i) / c->points.size());
  return c;
}

static int Gpu(int argc, char** argv) {
  if (argc < 6) return 2;
  const std::string dir = argv[2];
  const int scans = std::atoi(argv[3]), frame_count = std::atoi(argv[4]);
  bld::SubmapOptions opt;
  opt.frame_count = frame_count; opt.enable_voxel_filter = true; opt.voxel_size = 0.1f;
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
  be::LoopDetectorSettings s;
  s.loop_ignore_threshold = 2;
  s.use_descriptor = true;
  s.m2dp_match_score = static_cast<float>(std::atof(argv[5]));
  be::LoopDetector det(s);
  std::vector<std::shared_ptr<be::LoopFrame>> frames;
  std::printf("{\"status\": [");
  be::DetectResult last;
  for (size_t k = 0; k < maps.size(); ++k) {
    std::shared_ptr<be::LoopFrame> f(new be::LoopFrame);
    f->global_pose = maps[k]->FirstFramePose();
    if (!maps[k]->CalculateDescriptor()) return 3;                                             // the resident cloud, no download
    f->descriptor = maps[k]->GetDescriptor();
    f->cloud = maps[k]->Cloud();
    frames.push_back(f);
    last = det.AddFrame(f);
    std::printf("%s%d", k ? ", " : "", static_cast<int>(det.Status()));
  }
  std::printf("], \"scores\": [");
  for (size_t k = 0; k + 1 < frames.size(); ++k)
    std::printf("%s%.9f", k ? ", " : "", smhip::descriptor::matchTwoM2dpDescriptors(frames.back()->descriptor, frames[k]->descriptor));
  const be::LoopCandidates& c = det.LastCandidates();
  std::printf("], \"pairs\": [");
  for (size_t k = 0; k < c.maybe_close_pair.size(); ++k) std::printf("%s[%d, %d]", k ? ", " : "", c.maybe_close_pair[k].first, c.maybe_close_pair[k].second);
  // CloseLoop called directly on the same pairs, each with a matcher of its own
  std::vector<be::LoopEdge> direct;
  for (const auto& p : c.maybe_close_pair) {
    be::LoopEdge e;
    e.close_pair_index = p;
    const auto& t = frames[static_cast<size_t>(p.first)];
    const auto& src = frames[static_cast<size_t>(p.second)];
    if (be::CloseLoop(t->global_pose, t->cloud, src->global_pose, src->cloud, s, &e)) direct.push_back(e);
  }
  bool equal = direct.size() == last.edges.size();
  for (size_t k = 0; equal && k < direct.size(); ++k)
    equal = direct[k].close_pair_index == last.edges[k].close_pair_index && std::memcmp(direct[k].transform.m, last.edges[k].transform.m, sizeof(direct[k].transform.m)) == 0 &&
            std::memcmp(direct[k].init_guess.m, last.edges[k].init_guess.m, sizeof(direct[k].init_guess.m)) == 0 &&
            std::memcmp(&direct[k].score, &last.edges[k].score, sizeof(double)) == 0;
  std::printf("], \"edges\": [");
  for (size_t k = 0; k < last.edges.size(); ++k) {
    const be::LoopEdge& e = last.edges[k];
    std::printf("%s{\"target\": %d, \"source\": %d, \"score\": %.17g, \"transform\": [", k ? ", " : "", e.close_pair_index.first, e.close_pair_index.second, e.score);
    for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) std::printf("%.17g%s", e.transform(r, q), (r == 3 && q == 3) ? "" : ", ");
    std::printf("]}");
  }
  std::printf("], \"direct_edges\": %d, \"edges_equal_direct\": %s, \"close_succeed\": %s, \"last_status_before\": %d}\n", static_cast<int>(direct.size()),
              equal ? "true" : "false", last.close_succeed ? "true" : "false", static_cast<int>(last.status));
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "host") {
    CandidateChecks();
    MachineChecks();
    CheckResultChecks();
    std::printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
  }
  if (mode == "gpu") return Gpu(argc, argv);
  std::fprintf(stderr, "usage: test_loop_detector host | gpu <dir> <scans> <frame_count> <m2dp_match_score>\n");
  return 2;
}
