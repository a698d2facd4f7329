// The pose graph's PRIOR and POINT factors and IsamOptimizer's GPS bookkeeping: include/smhip/pose_graph.h, the host half of
// smhip_pose_graph_optimize_factors (csrc/pose_graph_plan.h) and the kernel's loop compiled for the CPU (csrc/pose_graph_kernel.h with
// HostCtx: one thread, empty barriers).
//   test_pose_graph_gps host             no device: the plan's counts, PoseGraph's arrays with the frame vertex last, Submap's ENU
//   test_pose_graph_gps solve IN OUT     the kernel's loop on the CPU for the problem in IN (see Solve), results to OUT
//   test_pose_graph_gps isam host|gpu IN IsamOptimizer over the hand-made frames of IN (see Isam), solved by the kernel's loop on the
//                                        CPU through the Solver hook, or on the device; one JSON line.  Exit 4: the options were refused
#define SMHIP_REGISTRATOR_THROW_ON_CHECK 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "smhip/pose_graph.h"
#include "../../staticmapping_amd/csrc/pose_graph_kernel.h"
#include "../../staticmapping_amd/csrc/pose_graph_plan.h"

namespace reg = smhip::registrator;
namespace bld = smhip::builder;
namespace be = smhip::back_end;
namespace pg = smhip::pose_graph;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static reg::Matrix4d Pose(double x, double y, double z, double yaw) {
  reg::Matrix4d p = reg::Matrix4d::Identity();
  p(0, 0) = std::cos(yaw); p(0, 1) = -std::sin(yaw); p(1, 0) = std::sin(yaw); p(1, 1) = std::cos(yaw);
  p(0, 3) = x; p(1, 3) = y; p(2, 3) = z;
  return p;
}

// ---- the kernel's loop on the CPU --------------------------------------------------------------------------------------------

struct HostProblem {
  int n = 0, m = 0;
  std::vector<double> pose0, Z, sinv, v;          // 12 n, 12 m, 6 m, 6 n
  std::vector<int32_t> fixed, ij, kind, csr_off, csr_edge;
  std::vector<double> work, out_d;
  std::vector<int32_t> out_i;
  pg::Dev d;

  // the node -> factors list as the library makes it (a PRIOR once), and the per-solve cap
  int MakeCsr() {
    const size_t N = static_cast<size_t>(n), M = static_cast<size_t>(m);
    csr_off.assign(N + 1, 0);
    int non_chain = 0;
    for (size_t e = 0; e < M; ++e) {
      const int i = ij[2 * e], j = ij[2 * e + 1];
      ++csr_off[static_cast<size_t>(i) + 1];
      if (j != i) ++csr_off[static_cast<size_t>(j) + 1];
      if (kind[e] != SMHIP_POSE_GRAPH_FACTOR_PRIOR && std::abs(i - j) != 1) ++non_chain;
    }
    for (size_t k = 0; k < N; ++k) csr_off[k + 1] += csr_off[k];
    csr_edge.assign(static_cast<size_t>(csr_off[N]), 0);
    std::vector<int32_t> at(csr_off.begin(), csr_off.end() - 1);
    for (size_t e = 0; e < M; ++e) {
      const int i = ij[2 * e], j = ij[2 * e + 1];
      csr_edge[static_cast<size_t>(at[static_cast<size_t>(i)]++)] = static_cast<int32_t>(e);
      if (j != i) csr_edge[static_cast<size_t>(at[static_cast<size_t>(j)]++)] = static_cast<int32_t>(e);
    }
    return 12 * non_chain + 64;
  }
  // sizes and inputs set: lay the work arrays out and point d at everything
  void Bind(int max_it, int pcg_cap) {
    const size_t N = static_cast<size_t>(n), M = static_cast<size_t>(m);
    work.assign(N * (2 * 12 + 7 * 36 + 7 * 6 + 6) + M * (2 * 36 + 2 * 6), std::numeric_limits<double>::quiet_NaN());   // (nothing may be read before it is written)
    out_d.assign(pg::kOutDoubles, 0.0);
    out_i.assign(pg::kOutInts, 0);
    if (v.empty()) v.assign(6 * N, 0.0);
    double* p = work.data();
    auto take = [&p](size_t c) { double* r = p; p += c; return r; };
    d.n = n; d.m = m; d.max_it = max_it; d.pcg_cap = pcg_cap; d.pcg_budget = SMHIP_POSE_GRAPH_MAX_PCG_TOTAL; d.probe = 0;
    d.pose0 = pose0.data(); d.Z = Z.data(); d.sinv = sinv.data(); d.v = v.data();
    d.fixed = fixed.data(); d.ij = ij.data(); d.kind = kind.data(); d.csr_off = csr_off.data(); d.csr_edge = csr_edge.data();
    d.cur = take(12 * N); d.cand = take(12 * N);
    d.Hkk = take(36 * N); d.C = take(36 * N); d.D = take(36 * N); d.U = take(36 * N); d.Dinv = take(36 * N); d.Wm = take(36 * N); d.Wp = take(36 * N);
    d.g = take(6 * N); d.x = take(6 * N); d.r = take(6 * N); d.z = take(6 * N); d.p = take(6 * N); d.q = take(6 * N); d.b = take(6 * N);
    d.minv = take(6 * N);
    d.A = take(36 * M); d.B = take(36 * M); d.rw = take(6 * M); d.u = take(6 * M);
    d.out_d = out_d.data(); d.out_i = out_i.data();
  }
};

static void Pack12(const double* m, double* o) {
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) o[3 * r + c] = m[4 * c + r]; o[9 + r] = m[12 + r]; }
}

static int g_host_solves = 0, g_last_nodes = 0, g_last_factors = 0, g_last_points = 0;
static int g_max_iterations = 50;

// IsamOptimizer's solver without a device: smhip_pose_graph_optimize_factors' host half, then the kernel's loop on this thread
static bool HostSolve(be::PoseGraph* graph) {
  std::vector<double> poses, data, sigmas;
  std::vector<int32_t> ij;
  std::vector<uint8_t> fixed, kinds;
  graph->FlattenFactors(&poses, &fixed, &kinds, &ij, &data, &sigmas);
  HostProblem hp;
  hp.n = graph->NodeCount(); hp.m = static_cast<int>(kinds.size());
  pg::Plan plan;
  std::string why;
  if (pg::check_and_plan_factors(hp.n, poses.data(), fixed.data(), hp.m, kinds.data(), ij.data(), data.data(), sigmas.data(), &plan, &why) != SMHIP_OK) {
    std::fprintf(stderr, "%s\n", why.c_str());
    return false;
  }
  const size_t N = static_cast<size_t>(hp.n), M = static_cast<size_t>(hp.m);
  hp.pose0.resize(12 * N); hp.Z.assign(12 * M, 0.0); hp.sinv.assign(6 * M, 0.0);
  for (size_t k = 0; k < N; ++k) Pack12(&poses[16 * k], &hp.pose0[12 * k]);
  for (size_t e = 0; e < M; ++e) {
    if (kinds[e] == SMHIP_POSE_GRAPH_FACTOR_POINT) {
      for (int c = 0; c < 6; ++c) hp.Z[12 * e + c] = data[16 * e + c];
      for (int c = 0; c < 3; ++c) hp.sinv[6 * e + c] = 1.0 / sigmas[6 * e + c];
    } else {
      Pack12(&data[16 * e], &hp.Z[12 * e]);
      for (int c = 0; c < 6; ++c) hp.sinv[6 * e + c] = 1.0 / sigmas[6 * e + c];
    }
  }
  hp.fixed.assign(fixed.begin(), fixed.end());
  hp.kind.assign(kinds.begin(), kinds.end());
  hp.ij = ij;
  const int cap = hp.MakeCsr();
  if (hp.csr_off != plan.csr_offsets || hp.csr_edge != plan.csr_edges || cap != plan.pcg_cap) { std::fprintf(stderr, "the plan's list differs\n"); return false; }
  hp.Bind(g_max_iterations, plan.pcg_cap);
  pg::HostCtx c;
  pg::run(hp.d, c);
  if (hp.out_i[pg::kOutStop] == SMHIP_POSE_GRAPH_STOP_NUMERIC) return false;
  for (size_t k = 0; k < N; ++k) {
    if (hp.fixed[k]) continue;
    const double* p = hp.d.cur + 12 * k;
    double* o = &poses[16 * k];
    for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) o[4 * q + r] = p[3 * r + q]; o[12 + r] = p[9 + r]; }
  }
  graph->SetFlatNodePoses(poses);
  ++g_host_solves; g_last_nodes = hp.n; g_last_factors = hp.m; g_last_points = graph->PointFactorCount();
  return true;
}

// IN: int32 n, m; then doubles pose0[12 n], Z[12 m] (as the device holds them: a POINT's lever and point first), sinv[6 m], v[6 n];
// then int32 fixed[n], ij[2 m], kind[m], max_it.  OUT: doubles cur[12 n], out_d[3], out_i[6] (as doubles), then of a second, probing
// run: rw[6 m], A[36 m], B[36 m], g[6 n], minv[6 n].
static int Solve(const char* in_path, const char* out_path) {
  std::ifstream in(in_path, std::ios::binary);
  HostProblem hp;
  int32_t nm[2];
  if (!in.read(reinterpret_cast<char*>(nm), sizeof(nm))) return 2;
  hp.n = nm[0]; hp.m = nm[1];
  const size_t N = static_cast<size_t>(hp.n), M = static_cast<size_t>(hp.m);
  hp.pose0.resize(12 * N); hp.Z.resize(12 * M); hp.sinv.resize(6 * M); hp.v.resize(6 * N); hp.fixed.resize(N); hp.ij.resize(2 * M); hp.kind.resize(M);
  int32_t max_it = 0;
  auto rd = [&in](void* p, size_t bytes) { return bytes == 0 || static_cast<bool>(in.read(reinterpret_cast<char*>(p), static_cast<std::streamsize>(bytes))); };
  if (!rd(hp.pose0.data(), 96 * N) || !rd(hp.Z.data(), 96 * M) || !rd(hp.sinv.data(), 48 * M) || !rd(hp.v.data(), 48 * N) || !rd(hp.fixed.data(), 4 * N) ||
      !rd(hp.ij.data(), 8 * M) || !rd(hp.kind.data(), 4 * M) || !rd(&max_it, 4))
    return 2;
  hp.Bind(max_it, hp.MakeCsr());
  pg::HostCtx c;
  pg::run(hp.d, c);
  std::ofstream out(out_path, std::ios::binary);
  auto wr = [&out](const void* p, size_t bytes) { out.write(reinterpret_cast<const char*>(p), static_cast<std::streamsize>(bytes)); };
  wr(hp.d.cur, 96 * N);
  wr(hp.out_d.data(), 8 * pg::kOutDoubles);
  std::vector<double> oi(hp.out_i.begin(), hp.out_i.end());
  wr(oi.data(), 8 * oi.size());
  hp.d.probe = 1;
  pg::run(hp.d, c);
  wr(hp.d.rw, 48 * M); wr(hp.d.A, 288 * M); wr(hp.d.B, 288 * M); wr(hp.d.g, 48 * N); wr(hp.d.minv, 48 * N);
  return out ? 0 : 2;
}

// ---- host checks ---------------------------------------------------------------------------------------------------------------

static void PlanAndGraphChecks() {
  // a chain 0 - 1 - 2 - 3 with a loop edge (0, 3), the frame vertex with its prior, a prior on vertex 2, points on vertices 1 and 3
  be::PoseGraph g;
  for (int k = 0; k < 4; ++k) g.AddVertex(k, Pose(k, 0.1 * k, 0, 0.2 * k), Pose(1, 0.1, 0, 0.2));
  g.AddLoopCloseEdge(0, 3, Pose(3, 0.3, 0, 0.6));
  EXPECT(!g.HasFactors() && g.NodeCount() == 4);
  const be::Sigmas tight = {0.01, 0.01, 0.01, 0.01, 0.01, 0.01};
  g.AddPriorFactor(2, Pose(2, 0.2, 0, 0.4), tight);
  g.SetFrameVertex(Pose(100, -50, 3, 0.4), be::GpsCoordPriorSigmas());
  const double lever[3] = {0.3, -0.2, 1.1}, p1[3] = {101, -49, 4}, p3[3] = {103, -48, 4};
  g.AddPointFactor(1, lever, p1, be::GpsSigmas());
  g.AddPointFactor(3, lever, p3, be::GpsSigmas());
  EXPECT(g.HasFactors() && g.NodeCount() == 5 && g.VertexCount() == 4 && g.Edges().size() == 4 && g.PointFactorCount() == 2);
  std::vector<double> poses, data, sigmas;
  std::vector<int32_t> ij;
  std::vector<uint8_t> fixed, kinds;
  g.FlattenFactors(&poses, &fixed, &kinds, &ij, &data, &sigmas);
  EXPECT(poses.size() == 80 && fixed == std::vector<uint8_t>({1, 0, 0, 0, 0}));
  EXPECT(kinds == std::vector<uint8_t>({0, 0, 0, 0, 1, 1, 2, 2}));
  EXPECT(ij == std::vector<int32_t>({0, 1, 1, 2, 2, 3, 0, 3, 4, 4, 2, 2, 4, 1, 4, 3}));          // the frame vertex is the last node
  EXPECT(poses[64 + 12] == 100.0 && data[16 * 4 + 12] == 100.0 && data[16 * 6] == 0.3 && data[16 * 7 + 3] == 103.0 && sigmas[6 * 6] == 0.15 && sigmas[6 * 4 + 2] == 0.2);
  pg::Plan plan;
  std::string why;
  EXPECT(pg::check_and_plan_factors(5, poses.data(), fixed.data(), 8, kinds.data(), ij.data(), data.data(), sigmas.data(), &plan, &why) == SMHIP_OK);
  // non-chain: the loop edge (0, 3) and the point (4, 1); the point (4, 3) lands in a chain block, the priors are never counted
  EXPECT(plan.non_chain_edges == 2 && plan.pcg_cap == 88 && plan.levels == 3);
  // node 0: 0 3 | node 1: 0 1 6 | node 2: 1 2 5 (its prior once) | node 3: 2 3 7 | node 4: 4 (its prior once) 6 7
  EXPECT(plan.csr_offsets == std::vector<int32_t>({0, 2, 5, 8, 11, 14}));
  EXPECT(plan.csr_edges == std::vector<int32_t>({0, 3, 0, 1, 6, 1, 2, 5, 2, 3, 7, 4, 6, 7}));
  // the same through the library's symbol; NULL kinds with the between-factors alone give the old plan
  std::vector<int32_t> off(6), edges(16);
  char text[128];
  EXPECT(smhip_pose_graph_plan_factors(5, poses.data(), fixed.data(), 8, kinds.data(), ij.data(), data.data(), sigmas.data(), off.data(), edges.data(), text, sizeof(text)) == SMHIP_OK);
  EXPECT(off == plan.csr_offsets && std::vector<int32_t>(edges.begin(), edges.begin() + 14) == plan.csr_edges);
  pg::Plan old_plan, null_plan;
  EXPECT(pg::check_and_plan(4, poses.data(), fixed.data(), 4, ij.data(), data.data(), sigmas.data(), &old_plan, nullptr) == SMHIP_OK);
  EXPECT(pg::check_and_plan_factors(4, poses.data(), fixed.data(), 4, nullptr, ij.data(), data.data(), nullptr, &null_plan, nullptr) == SMHIP_OK);
  EXPECT(old_plan.csr_offsets == null_plan.csr_offsets && old_plan.csr_edges == null_plan.csr_edges && old_plan.pcg_cap == null_plan.pcg_cap && old_plan.non_chain_edges == 1);
  // null sigmas with another kind present are refused
  EXPECT(pg::check_and_plan_factors(5, poses.data(), fixed.data(), 8, kinds.data(), ij.data(), data.data(), nullptr, nullptr, &why) == SMHIP_ERR_INVALID_ARGUMENT && !why.empty());
  // solved by the kernel's loop: the frame vertex comes back, the first vertex is where it was
  const reg::Matrix4d first = g.Pose(0);
  EXPECT(HostSolve(&g) && g_last_nodes == 5 && g_last_factors == 8);
  EXPECT(std::memcmp(first.m, g.Pose(0).m, sizeof(first.m)) == 0);
  EXPECT(std::fabs(g.FrameVertexPose()(0, 3) - 100.0) < 5.0 && g.FrameVertexPose()(0, 3) != 100.0);
}

static void SubmapEnuChecks() {
  bld::SubmapOptions opt;
  bld::Submap s(opt);
  EXPECT(!s.HasGps());
  s.SetRelatedGpsInENU(1.5, -2.5, 3.5);
  EXPECT(s.HasGps() && s.GetRelatedGpsInENU()[0] == 1.5 && s.GetRelatedGpsInENU()[1] == -2.5 && s.GetRelatedGpsInENU()[2] == 3.5);
  be::LoopFrame f;
  EXPECT(!f.has_enu && f.enu[2] == 0.0);
  be::IsamOptimizerOptions o;
  EXPECT(!o.use_gps && o.gps_factor_init_num == 25 && o.gps_factor_sample_step == 1 && o.gps_factor_init_angle_rad == 1.6 && !o.enable_extrinsic_calib);
  be::IsamOptimizer plain(o, be::LoopDetectorSettings(), nullptr);
  const reg::Matrix4d I = reg::Matrix4d::Identity();
  EXPECT(std::memcmp(plain.GetGpsCoordTransform().m, I.m, sizeof(I.m)) == 0 && plain.GpsFactorCount() == 0);
}

// ---- IsamOptimizer over hand-made frames ------------------------------------------------------------------------------------------

// IN (text): use_gps init_num sample_step init_angle extrinsic; lever x y z; n; then per frame 16 doubles of the fed pose (row-major),
// has_enu, east north up.  The odometry factor of frame k is the fed poses' own step.
static int Isam(const std::string& where, const char* path) {
  std::ifstream in(path);
  be::IsamOptimizerOptions o;
  int use_gps = 0, extrinsic = 0, n = 0;
  double lever[3];
  if (!(in >> use_gps >> o.gps_factor_init_num >> o.gps_factor_sample_step >> o.gps_factor_init_angle_rad >> extrinsic >> lever[0] >> lever[1] >> lever[2] >> n)) return 2;
  o.use_gps = use_gps != 0; o.enable_extrinsic_calib = extrinsic != 0;
  std::vector<std::shared_ptr<be::LoopFrame>> frames;
  for (int k = 0; k < n; ++k) {
    std::shared_ptr<be::LoopFrame> f(new be::LoopFrame);
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) in >> f->global_pose(r, c);
    int has = 0;
    in >> has >> f->enu[0] >> f->enu[1] >> f->enu[2];
    f->has_enu = has != 0;
    frames.push_back(f);
  }
  if (!in) return 2;
  be::LoopDetectorSettings lds;                      // the drive never comes within 25 m of a frame older than 15: the detector finds nothing
  std::unique_ptr<be::IsamOptimizer> opt;
  std::shared_ptr<smhip::pre_processers::filter::DeviceContext> context;
  try {
    if (where == "gpu") {
      context = smhip::pre_processers::filter::DeviceContext::Default();
      opt.reset(new be::IsamOptimizer(o, lds, context->handle()));
    } else {
      opt.reset(new be::IsamOptimizer(o, lds, nullptr));
      opt->SetSolver(HostSolve);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 4;
  }
  reg::Matrix4d tracking_to_gps = Pose(lever[0], lever[1], lever[2], 0.7);                      // (only its translation is used)
  opt->SetTransformTrackingToGps(tracking_to_gps);
  std::vector<reg::Matrix4d> odoms;
  for (int k = 0; k < n; ++k) odoms.push_back(k == 0 ? reg::Matrix4d::Identity() : be::Multiply(be::RigidInverse(frames[k - 1]->global_pose), frames[k]->global_pose));
  std::printf("{\"angles\": [");
  bool all_ok = true;
  for (int k = 0; k < n; ++k) {
    frames[k]->cloud.reset();
    // what AnalyseAllFramePoseForMaxRotation will see for this frame: the frames so far at their current poses and this one as fed
    std::vector<reg::Matrix4d> seen;
    for (int q = 0; q <= k; ++q) seen.push_back(frames[q]->global_pose);
    double most = 0.0;
    for (const auto& p : seen) {
      double dot = seen[0](0, 0) * p(0, 0) + seen[0](1, 0) * p(1, 0) + seen[0](2, 0) * p(2, 0);
      dot = dot > 1.0 ? 1.0 : dot < -1.0 ? -1.0 : dot;
      most = std::fmax(most, std::fabs(std::acos(dot)));
    }
    std::printf("%s%.17g", k ? ", " : "", k == 0 ? 0.0 : most);
    be::DetectResult r;
    r.current_frame_index = k;
    all_ok = opt->AddDetected(frames[k], odoms[k], r) && all_ok;
  }
  all_ok = opt->RunFinalOptimazation() && all_ok;
  std::printf("], \"ok\": %s, \"gps_factors\": %d, \"cached\": %d, \"solves\": %d, \"factor_indices\": [", all_ok ? "true" : "false", opt->GpsFactorCount(),
              opt->CachedEnuCount(), opt->SolveCount());
  bool first = true;
  for (const auto& f : opt->Graph().Factors())
    if (f.kind == SMHIP_POSE_GRAPH_FACTOR_POINT) { std::printf("%s%d", first ? "" : ", ", f.index); first = false; }
  const smhip_pose_graph_stats& st = opt->LastStats();
  const smhip_pose_graph_stats& al = opt->AloneStats();
  std::printf("], \"stop_reason\": %d, \"pcg_max_iterations\": %d, \"alone_stop_reason\": %d, \"alone_accepted\": %d, \"alone_rejected\": %d, \"alone_pcg_max\": %d, \"nodes\": %d, \"gps_coord\": [",
              st.stop_reason, st.pcg_max_iterations, al.stop_reason, al.accepted_steps, al.rejected_steps, al.pcg_max_iterations, opt->Graph().NodeCount());
  const reg::Matrix4d G = opt->GetGpsCoordTransform();
  for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) std::printf("%.17g%s", G(r, q), (r == 3 && q == 3) ? "" : ", ");
  std::printf("], \"poses\": [");
  for (int k = 0; k < n; ++k) {
    std::printf("%s[", k ? ", " : "");
    for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) std::printf("%.17g%s", frames[k]->global_pose(r, q), (r == 3 && q == 3) ? "" : ", ");
    std::printf("]");
  }
  std::printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "host") {
    PlanAndGraphChecks();
    SubmapEnuChecks();
    std::printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
  }
  if (mode == "solve" && argc == 4) return Solve(argv[2], argv[3]);
  if (mode == "isam" && argc == 4) return Isam(argv[2], argv[3]);
  std::fprintf(stderr, "usage: test_pose_graph_gps host | solve IN OUT | isam host|gpu IN\n");
  return 2;
}
