// LoopDetectorSettings::guess_search (include/smhip/back_end.h): the correlative guess search in front of CloseLoop's ICP.
//   test_loop_guess_search host        no device: a scan matcher whose Align records where it starts and a hook in place of the search --
//                                      the searched guess is used only when it scores above the guess, the edge's new fields, a refused
//                                      search fails the pair, and with the setting off nothing is searched
//   test_loop_guess_search gpu <dir>   <dir>/target.bin, <dir>/source.bin (KITTI scans) and <dir>/poses.txt (two row-major 4x4: the
//                                      target's global pose and the source's DRIFTED one): CloseLoop with the search on and off; one
//                                      JSON line
#define SMHIP_REGISTRATOR_THROW_ON_CHECK 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "smhip/back_end.h"

namespace reg = smhip::registrator;
namespace be = smhip::back_end;
using smhip::data::InnerPointCloudData;
using smhip::data::InnerPointType;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static reg::Matrix4d Pose(double x, double y, double z, double yaw) {
  reg::Matrix4d p = reg::Matrix4d::Identity();
  p(0, 0) = std::cos(yaw); p(0, 1) = -std::sin(yaw); p(1, 0) = std::sin(yaw); p(1, 1) = std::cos(yaw);
  p(0, 3) = x; p(1, 3) = y; p(2, 3) = z;
  return p;
}
static bool Same(const reg::Matrix4d& a, const reg::Matrix4d& b) { return std::memcmp(a.data(), b.data(), sizeof(double) * 16) == 0; }

static be::InnerCloudPtr Cloud(int n, float x0) {
  std::vector<InnerPointType> pts(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) { pts[i].x = x0 + i; pts[i].y = 0.5f * i; pts[i].z = 0.f; pts[i].intensity = 1.f; pts[i].factor = 0.f; }
  return be::InnerCloudPtr(new InnerPointCloudData(pts));
}

// no device: Align ends where it starts and scores 0.9
struct RecordingMatcher : reg::IcpPointMatcherHip {
  int aligns = 0, own_searches = 0;
  reg::Matrix4d started_from = reg::Matrix4d::Identity();
  void InitWithOptions() override {}
  void SetInputSource(InnerCloudPtr) override {}
  void SetInputTarget(InnerCloudPtr) override {}
  bool Align(const reg::Matrix4d& guess, reg::Matrix4d& result) override { ++aligns; started_from = guess; result = guess; this->final_score_ = 0.9; return true; }
  bool GuessSearch(const InnerCloudPtr&, const InnerCloudPtr&, const reg::Matrix4d& guess, const smhip_guess_search_options&, smhip_guess_search_result* out) override {
    ++own_searches;
    std::memset(out, 0, sizeof(*out));
    std::memcpy(out->transform, guess.data(), sizeof(double) * 16);
    out->transform[12] += 1.0;
    out->best_score = 3; out->guess_score = 1; out->runner_up_score = 2;
    return true;
  }
};

struct Hook {
  int calls = 0, best = 0, guess = 0, runner_up = 0;
  bool ok = true;
  reg::Matrix4d answer = reg::Matrix4d::Identity(), seen_guess = reg::Matrix4d::Identity();
  smhip_guess_search_options seen_options{};
  be::InnerCloudPtr seen_target, seen_source;
  be::GuessSearcher Function() {
    return [this](const be::InnerCloudPtr& t, const be::InnerCloudPtr& s, const reg::Matrix4d& g, const smhip_guess_search_options& o, smhip_guess_search_result* out) {
      ++calls; seen_guess = g; seen_options = o; seen_target = t; seen_source = s;
      if (!ok) return false;
      std::memset(out, 0, sizeof(*out));
      std::memcpy(out->transform, answer.data(), sizeof(double) * 16);
      out->best_score = best; out->guess_score = guess; out->runner_up_score = runner_up;
      return true;
    };
  }
};

struct OpenDetector : be::LoopDetector {
  using be::LoopDetector::LoopDetector;
  bool Close(be::LoopEdge* e) { return CloseLoopPair(e); }
};

static int Host() {
  const reg::Matrix4d target_pose = Pose(3, -2, 0.7, 0.3), source_pose = Pose(9, 4, 1.9, 0.5);
  reg::Matrix4d pose_guess = be::Multiply(be::RigidInverse(target_pose), source_pose);
  EXPECT(pose_guess(2, 3) != 0.0);
  pose_guess(2, 3) = 0.0;                                                   // loop_detector.cc:290
  const be::InnerCloudPtr target = Cloud(5, 0.f), source = Cloud(4, 1.f);
  const reg::Matrix4d found = Pose(-1.5, 2.5, 0.5, 0.1);

  be::LoopDetectorSettings off;
  EXPECT(!off.guess_search);                                                // opt-in
  EXPECT(off.guess_search_options.resolution == 0.5f && off.guess_search_options.max_source_points == 4096 && off.guess_search_options.half_xy == 20 &&
         off.guess_search_options.half_z == 2 && off.guess_search_options.yaw_steps == 10 && std::fabs(off.guess_search_options.yaw_step - 2.0 * M_PI / 180.0) < 1e-15);
  be::LoopDetectorSettings on = off;
  on.guess_search = true;
  on.guess_search_options.half_xy = 7; on.guess_search_options.resolution = 0.25f;

  {  // off: nothing is searched, the edge is what it was
    RecordingMatcher m; Hook h; h.best = 9; h.guess = 1; h.answer = found;
    const be::GuessSearcher f = h.Function();
    be::LoopEdge e, plain;
    EXPECT(be::CloseLoop(target_pose, target, source_pose, source, off, &e, &m, &f));
    EXPECT(h.calls == 0 && m.own_searches == 0 && m.aligns == 1 && Same(m.started_from, pose_guess));
    RecordingMatcher m2;
    EXPECT(be::CloseLoop(target_pose, target, source_pose, source, off, &plain, &m2));
    EXPECT(Same(e.init_guess, plain.init_guess) && Same(e.transform, plain.transform) && e.score == plain.score && Same(e.init_guess, pose_guess));
    EXPECT(!e.search_used && e.search_score == 0 && e.guess_score == 0 && e.runner_up_score == 0 && Same(e.searched_guess, reg::Matrix4d::Identity()));
    EXPECT(std::fabs(e.score + std::log(0.9)) < 1e-15);
  }
  {  // on, the search beats the guess: the ICP starts from what it found; init_guess stays the pose-derived one
    RecordingMatcher m; Hook h; h.best = 10; h.guess = 4; h.runner_up = 6; h.answer = found;
    const be::GuessSearcher f = h.Function();
    be::LoopEdge e;
    EXPECT(be::CloseLoop(target_pose, target, source_pose, source, on, &e, &m, &f));
    EXPECT(h.calls == 1 && m.own_searches == 0 && m.aligns == 1);
    EXPECT(Same(h.seen_guess, pose_guess));                                 // searched from init_guess, after the z = 0 line
    EXPECT(h.seen_options.half_xy == 7 && h.seen_options.resolution == 0.25f && h.seen_options.yaw_steps == 10);
    EXPECT(h.seen_target == target && h.seen_source == source);
    EXPECT(Same(m.started_from, found) && Same(e.transform, found));
    EXPECT(Same(e.init_guess, pose_guess) && Same(e.searched_guess, found));
    EXPECT(e.search_used && e.search_score == 10 && e.guess_score == 4 && e.runner_up_score == 6);
  }
  for (int best : {7, 6}) {  // on, the search does not beat the guess (equal, lower): the ICP starts from the guess, the fields are still filled
    RecordingMatcher m; Hook h; h.best = best; h.guess = 7; h.runner_up = 7; h.answer = found;
    const be::GuessSearcher f = h.Function();
    be::LoopEdge e;
    EXPECT(be::CloseLoop(target_pose, target, source_pose, source, on, &e, &m, &f));
    EXPECT(h.calls == 1 && Same(m.started_from, pose_guess) && Same(e.transform, pose_guess));
    EXPECT(!e.search_used && e.search_score == best && e.guess_score == 7 && e.runner_up_score == 7 && Same(e.searched_guess, found));
  }
  {  // a refused search fails the pair before any alignment
    RecordingMatcher m; Hook h; h.ok = false;
    const be::GuessSearcher f = h.Function();
    be::LoopEdge e;
    EXPECT(!be::CloseLoop(target_pose, target, source_pose, source, on, &e, &m, &f));
    EXPECT(h.calls == 1 && m.aligns == 0 && !e.search_used && Same(e.init_guess, pose_guess));
  }
  {  // no hook (null, or an empty function): the matcher's own search
    RecordingMatcher m;
    be::LoopEdge e;
    EXPECT(be::CloseLoop(target_pose, target, source_pose, source, on, &e, &m));
    EXPECT(m.own_searches == 1 && e.search_used && e.search_score == 3 && e.guess_score == 1 && e.runner_up_score == 2);
    EXPECT(m.started_from(0, 3) == pose_guess(0, 3) + 1.0);
    const be::GuessSearcher empty;
    be::LoopEdge e2;
    EXPECT(be::CloseLoop(target_pose, target, source_pose, source, on, &e2, &m, &empty));
    EXPECT(m.own_searches == 2);
  }
  for (bool search : {false, true}) {  // LoopDetector::CloseLoopPair hands its hook on
    be::LoopDetectorSettings s = search ? on : off;
    OpenDetector det(s);
    auto* m = new RecordingMatcher;
    det.SetScanMatcher(std::unique_ptr<reg::IcpPointMatcherHip>(m));
    Hook h; h.best = 5; h.guess = 2; h.runner_up = 1; h.answer = found;
    det.SetGuessSearcher(h.Function());
    auto a = std::make_shared<be::LoopFrame>(), b = std::make_shared<be::LoopFrame>();
    a->global_pose = target_pose; a->cloud = target; b->global_pose = source_pose; b->cloud = source;
    det.AddFrame(a, false); det.AddFrame(b, false);
    be::LoopEdge e;
    e.close_pair_index = {0, 1};
    EXPECT(det.Close(&e));
    EXPECT(h.calls == (search ? 1 : 0) && m->aligns == 1 && m->own_searches == 0);
    EXPECT(e.search_used == search && Same(m->started_from, search ? found : pose_guess) && Same(e.init_guess, pose_guess));
    EXPECT(e.search_score == (search ? 5 : 0) && e.guess_score == (search ? 2 : 0) && e.runner_up_score == (search ? 1 : 0));
  }
  if (failures) { std::printf("%d checks FAILED\n", failures); return 1; }
  std::printf("all checks passed\n");
  return 0;
}

static be::InnerCloudPtr ReadKittiBin(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<InnerPointType> pts;
  float row[4];
  while (f.read(reinterpret_cast<char*>(row), sizeof(row))) { InnerPointType p; p.x = row[0]; p.y = row[1]; p.z = row[2]; p.intensity = row[3]; p.factor = 0.f; pts.push_back(p); }
  return be::InnerCloudPtr(new InnerPointCloudData(pts));
}

static void PrintMatrix(const char* name, const reg::Matrix4d& T, const char* tail) {
  std::printf("\"%s\": [", name);
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) std::printf("%s%.17g", r + c ? ", " : "", T(r, c));
  std::printf("]%s", tail);
}

static int Gpu(int argc, char** argv) {
  if (argc < 3) return 2;
  const std::string dir = argv[2];
  const be::InnerCloudPtr target = ReadKittiBin(dir + "/target.bin"), source = ReadKittiBin(dir + "/source.bin");
  std::ifstream pf(dir + "/poses.txt");
  reg::Matrix4d P[2];
  for (auto& M : P) for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) pf >> M(r, c);
  be::LoopDetectorSettings s;
  be::LoopEdge on, off;
  s.guess_search = true;
  const bool ok_on = be::CloseLoop(P[0], target, P[1], source, s, &on);
  s.guess_search = false;
  const bool ok_off = be::CloseLoop(P[0], target, P[1], source, s, &off);
  std::printf("{\"accepted_on\": %s, \"accepted_off\": %s, \"search_used\": %s, \"search_score\": %d, \"guess_score\": %d, \"runner_up_score\": %d, \"score_on\": %.9g, \"score_off\": %.9g, ",
              ok_on ? "true" : "false", ok_off ? "true" : "false", on.search_used ? "true" : "false", on.search_score, on.guess_score, on.runner_up_score, on.score, off.score);
  PrintMatrix("init_guess", on.init_guess, ", ");
  PrintMatrix("searched_guess", on.searched_guess, ", ");
  PrintMatrix("transform_on", on.transform, ", ");
  PrintMatrix("transform_off", off.transform, ", ");
  std::printf("\"off_untouched\": %s}\n", (!off.search_used && off.search_score == 0 && Same(off.init_guess, on.init_guess)) ? "true" : "false");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  try {
    if (mode == "host") return Host();
    if (mode == "gpu") return Gpu(argc, argv);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "exception: %s\n", e.what());
    return 3;
  }
  std::fprintf(stderr, "usage: test_loop_guess_search host | gpu <dir>\n");
  return 2;
}
