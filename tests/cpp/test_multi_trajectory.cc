// include/smhip/multi_trajectory.h: MultiTrajectoryOptimizer and MultiTrajectoryMapBuilder.
//   test_multi_trajectory host FIXTURE_XML TMPDIR     no device: the factor list of a 3 + 2 join against a list written out here, the plan
//                                                     accepting it free and held, the refusals, the search window, the solve count, the
//                                                     builder's index offsets, all through the Solver hook
//   test_multi_trajectory graph host|gpu IN           a join fed by hand (see Graph) solved by the kernel's loop on the CPU through the
//                                                     Solver hook, or on the device; one JSON line
//   test_multi_trajectory base host|gpu MAP_XML       LoadBaseMap, then a forced solve: one JSON line with the costs and whether a bit moved
//   test_multi_trajectory join gpu BASE INC OUT HOLD M2DP_SCORE [PCD STATIC]   the builder end to end on the device; one JSON line
#define SMHIP_REGISTRATOR_THROW_ON_CHECK 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "smhip/multi_trajectory.h"
#include "../../staticmapping_amd/csrc/pose_graph_kernel.h"
#include "../../staticmapping_amd/csrc/pose_graph_plan.h"

namespace reg = smhip::registrator;
namespace be = smhip::back_end;
namespace bld = smhip::builder;
namespace pg = smhip::pose_graph;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static reg::Matrix4d Pose(double x, double y, double z, double yaw) {
  reg::Matrix4d p = reg::Matrix4d::Identity();
  p(0, 0) = std::cos(yaw); p(0, 1) = -std::sin(yaw); p(1, 0) = std::sin(yaw); p(1, 1) = std::cos(yaw);
  p(0, 3) = x; p(1, 3) = y; p(2, 3) = z;
  return p;
}

// ---- the kernel's loop on the CPU (as tests/cpp/test_pose_graph_robust.cc runs it) ---------------------------------------------

struct HostProblem {
  int n = 0, m = 0;
  std::vector<double> pose0, Z, sinv, v, huber;
  std::vector<int32_t> fixed, ij, kind, csr_off, csr_edge;
  std::vector<double> work, out_d;
  std::vector<int32_t> out_i;
  pg::Dev d;
  void Bind(int max_it, int pcg_cap) {
    const size_t N = static_cast<size_t>(n), M = static_cast<size_t>(m);
    work.assign(N * (2 * 12 + 7 * 36 + 7 * 6 + 6) + M * (2 * 36 + 2 * 6 + 3), std::numeric_limits<double>::quiet_NaN());
    out_d.assign(pg::kOutDoubles, 0.0);
    out_i.assign(pg::kOutInts, 0);
    v.assign(6 * N, 0.0);
    double* p = work.data();
    auto take = [&p](size_t c) { double* r = p; p += c; return r; };
    d.n = n; d.m = m; d.max_it = max_it; d.pcg_cap = pcg_cap; d.pcg_budget = SMHIP_POSE_GRAPH_MAX_PCG_TOTAL; d.probe = 0;
    d.pose0 = pose0.data(); d.Z = Z.data(); d.sinv = sinv.data(); d.v = v.data();
    d.huber = huber.empty() ? nullptr : huber.data();
    d.fixed = fixed.data(); d.ij = ij.data(); d.kind = kind.data(); d.csr_off = csr_off.data(); d.csr_edge = csr_edge.data();
    d.cur = take(12 * N); d.cand = take(12 * N);
    d.Hkk = take(36 * N); d.C = take(36 * N); d.D = take(36 * N); d.U = take(36 * N); d.Dinv = take(36 * N); d.Wm = take(36 * N); d.Wp = take(36 * N);
    d.g = take(6 * N); d.x = take(6 * N); d.r = take(6 * N); d.z = take(6 * N); d.p = take(6 * N); d.q = take(6 * N); d.b = take(6 * N);
    d.minv = take(6 * N);
    d.A = take(36 * M); d.B = take(36 * M); d.rw = take(6 * M); d.u = take(6 * M);
    d.wgt = take(M); d.rep_s = take(M); d.rep_c = take(M);
    d.out_d = out_d.data(); d.out_i = out_i.data();
  }
};

static void Pack12(const double* m, double* o) {
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) o[3 * r + c] = m[4 * c + r]; o[9 + r] = m[12 + r]; }
}

static bool Load(const be::PoseGraph& graph, HostProblem* hp, std::vector<double>* poses16) {
  std::vector<double> data, sigmas, huber;
  std::vector<int32_t> ij;
  std::vector<uint8_t> fixed, kinds;
  graph.FlattenFactors(poses16, &fixed, &kinds, &ij, &data, &sigmas);
  graph.FlattenHuber(&huber);
  hp->n = graph.NodeCount(); hp->m = static_cast<int>(kinds.size());
  pg::Plan plan;
  std::string why;
  if (pg::check_and_plan_robust(hp->n, poses16->data(), fixed.data(), hp->m, kinds.data(), ij.data(), data.data(), sigmas.data(), huber.data(), &plan, &why) != SMHIP_OK) {
    std::fprintf(stderr, "%s\n", why.c_str());
    return false;
  }
  const size_t N = static_cast<size_t>(hp->n), M = static_cast<size_t>(hp->m);
  hp->pose0.resize(12 * N); hp->Z.assign(12 * M, 0.0); hp->sinv.assign(6 * M, 0.0);
  for (size_t k = 0; k < N; ++k) Pack12(&(*poses16)[16 * k], &hp->pose0[12 * k]);
  for (size_t e = 0; e < M; ++e) {
    Pack12(&data[16 * e], &hp->Z[12 * e]);                                 // (BETWEEN and PRIOR alone: a join has no POINT factor)
    for (int c = 0; c < 6; ++c) hp->sinv[6 * e + c] = 1.0 / sigmas[6 * e + c];
  }
  hp->fixed.assign(fixed.begin(), fixed.end());
  hp->kind.assign(kinds.begin(), kinds.end());
  hp->ij = ij;
  if (graph.HasHuber()) hp->huber = huber;
  hp->csr_off = plan.csr_offsets; hp->csr_edge = plan.csr_edges;
  hp->Bind(50, plan.pcg_cap);
  return true;
}

static smhip_pose_graph_stats g_host_stats{};
static int g_host_solves = 0;

static bool HostSolve(be::PoseGraph* graph) {
  HostProblem hp;
  std::vector<double> poses;
  if (!Load(*graph, &hp, &poses)) return false;
  pg::HostCtx c;
  pg::run(hp.d, c);
  smhip_pose_graph_stats& s = g_host_stats;
  s.initial_cost = hp.out_d[0]; s.final_cost = hp.out_d[1]; s.damping = hp.out_d[2];
  s.stop_reason = hp.out_i[pg::kOutStop]; s.iterations = hp.out_i[1]; s.accepted_steps = hp.out_i[2]; s.rejected_steps = hp.out_i[3];
  s.pcg_iterations = hp.out_i[4]; s.pcg_max_iterations = hp.out_i[5];
  if (s.stop_reason == SMHIP_POSE_GRAPH_STOP_NUMERIC) return false;
  for (size_t k = 0; k < static_cast<size_t>(hp.n); ++k) {
    if (hp.fixed[k]) continue;
    const double* p = hp.d.cur + 12 * k;
    double* o = &poses[16 * k];
    for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) o[4 * q + r] = p[3 * r + q]; o[12 + r] = p[9 + r]; }
  }
  graph->SetFlatNodePoses(poses);
  ++g_host_solves;
  return true;
}

static bool HostReport(const be::PoseGraph& graph, std::vector<double>* norm, std::vector<double>* weight) {
  HostProblem hp;
  std::vector<double> poses;
  if (!Load(graph, &hp, &poses)) return false;
  for (size_t k = 0; k < 12 * static_cast<size_t>(hp.n); ++k) hp.d.cur[k] = hp.pose0[k];
  hp.d.probe = 2;
  pg::HostCtx c;
  pg::run(hp.d, c);
  norm->assign(hp.d.rep_s, hp.d.rep_s + hp.m);
  weight->assign(hp.d.wgt, hp.d.wgt + hp.m);
  return true;
}

// ---- host checks ---------------------------------------------------------------------------------------------------------------

static std::shared_ptr<be::LoopFrame> Frame(const reg::Matrix4d& pose) {
  std::shared_ptr<be::LoopFrame> f(new be::LoopFrame);
  f->global_pose = pose;
  return f;
}
static bld::SubmapId Id(int t, int s) { bld::SubmapId id; id.trajectory_index = t; id.submap_index = s; return id; }
static be::DetectResult Detected(int current, const std::vector<std::pair<int, reg::Matrix4d>>& edges) {
  be::DetectResult r;
  r.current_frame_index = current;
  for (const auto& e : edges) { be::LoopEdge le; le.close_pair_index = {e.first, current}; le.transform = e.second; r.edges.push_back(le); }
  r.close_succeed = !edges.empty();
  return r;
}

// trajectories of 3 and 2 submaps, two hand-made cross edges: (0,1) -> (1,0) and (0,2) -> (1,1)
static const double kBase[3][4] = {{0, 0, 0, 0}, {4, 0.5, 0.1, 0.1}, {8, 1.5, 0.2, 0.2}};
static const double kInc[2][4] = {{4.5, 1.0, 0.1, 0.15}, {8.5, 2.2, 0.2, 0.25}};
static const double kMoved[4] = {-0.3, -0.25, 0.02, -0.01};       // where the cross edges put the incremental map: this, times its loaded poses
static reg::Matrix4d CrossEdge(int k) {
  auto P = [](const double* v) { return Pose(v[0], v[1], v[2], v[3]); };
  return be::Multiply(be::RigidInverse(P(kBase[1 + k])), be::Multiply(P(kMoved), P(kInc[k])));
}

static bool FeedThreeAndTwo(be::MultiTrajectoryOptimizer* opt) {
  auto P = [](const double* v) { return Pose(v[0], v[1], v[2], v[3]); };
  bool ok = true;
  for (int k = 0; k < 3; ++k) ok = opt->AddDetected(Frame(P(kBase[k])), Id(0, k), Detected(k, {})) && ok;
  for (int k = 0; k < 2; ++k) ok = opt->AddSubmapConnection(Id(0, k), Id(0, k + 1), be::Multiply(be::RigidInverse(P(kBase[k])), P(kBase[k + 1])), false) && ok;
  EXPECT(opt->GetLoopDetector()->SearchWindow() == std::make_pair(-1, -1));
  opt->UseCurrentStateAsBaseMap();
  for (int k = 0; k < 2; ++k) ok = opt->AddDetected(Frame(P(kInc[k])), Id(1, k), Detected(3 + k, {{1 + k, CrossEdge(k)}})) && ok;
  ok = opt->AddSubmapConnection(Id(1, 0), Id(1, 1), be::Multiply(be::RigidInverse(P(kInc[0])), P(kInc[1])), false) && ok;
  return ok;
}

struct Want { int kind, i, j; const double* at; int from; double sigma, huber; };   // data: Pose(at); for from >= 0 the connection from that row's pose to Pose(at); at null: CrossEdge(from)

static void FactorList(bool hold) {
  be::MultiTrajectoryOptions o;
  o.hold_base_map = hold;
  EXPECT(o.loop_closure_huber == 1.0 && o.connection_huber == 0.0);
  be::MultiTrajectoryOptimizer opt(o, be::LoopDetectorSettings(), nullptr);
  opt.SetSolver(HostSolve);
  opt.SetReporter(HostReport);
  EXPECT(FeedThreeAndTwo(&opt));
  EXPECT(opt.GetLoopDetector()->SearchWindow() == std::make_pair(0, 2));              // (0, n_base - 1): the last base submap is never a candidate
  EXPECT(opt.BaseNodeCount() == 3 && opt.TrajectoryCount() == 2 && opt.SubmapCount(0) == 3 && opt.SubmapCount(1) == 2 && opt.LoopEdgeCount() == 2);
  EXPECT(opt.NodeOf(Id(0, 2)) == 2 && opt.NodeOf(Id(1, 0)) == 3 && opt.NodeOf(Id(1, 1)) == 4 && opt.NodeOf(Id(1, 2)) == -1 && opt.NodeOf(Id(2, 0)) == -1);
  EXPECT(opt.LoopConnections(Id(0, 1)) == std::vector<bld::SubmapId>({Id(1, 0)}) && opt.LoopConnections(Id(0, 2)) == std::vector<bld::SubmapId>({Id(1, 1)}) &&
         opt.LoopConnections(Id(0, 0)).empty() && opt.LoopConnections(Id(1, 1)).empty());
  std::vector<double> poses, data, sigmas, huber;
  std::vector<int32_t> ij;
  std::vector<uint8_t> fixed, kinds;
  opt.Graph().FlattenFactors(&poses, &fixed, &kinds, &ij, &data, &sigmas);
  opt.Graph().FlattenHuber(&huber);
  // the list, written out: the between-factors in the order added, then the priors
  std::vector<Want> want = {
      {SMHIP_POSE_GRAPH_FACTOR_BETWEEN, 0, 1, kBase[1], 0, 0.01, 0.0},   {SMHIP_POSE_GRAPH_FACTOR_BETWEEN, 1, 2, kBase[2], 1, 0.01, 0.0},
      {SMHIP_POSE_GRAPH_FACTOR_BETWEEN, 1, 3, nullptr, 0, 0.025, 1.0},    {SMHIP_POSE_GRAPH_FACTOR_BETWEEN, 2, 4, nullptr, 1, 0.025, 1.0},
      {SMHIP_POSE_GRAPH_FACTOR_BETWEEN, 3, 4, kInc[1], 10, 0.01, 0.0}};
  if (!hold) want.push_back({SMHIP_POSE_GRAPH_FACTOR_PRIOR, 0, 0, kBase[0], -1, 0.1, 0.0});
  want.push_back({SMHIP_POSE_GRAPH_FACTOR_PRIOR, 3, 3, kInc[0], -1, 0.1, 0.0});
  EXPECT(kinds.size() == want.size() && opt.Graph().FactorCount() == static_cast<int>(want.size()) && opt.Graph().NodeCount() == 5);
  for (size_t f = 0; f < want.size() && f < kinds.size(); ++f) {
    const Want& w = want[f];
    reg::Matrix4d d = w.at ? Pose(w.at[0], w.at[1], w.at[2], w.at[3]) : CrossEdge(w.from);
    if (w.at && w.from >= 0) { const double* a = w.from >= 10 ? kInc[w.from - 10] : kBase[w.from]; d = be::Multiply(be::RigidInverse(Pose(a[0], a[1], a[2], a[3])), d); }
    EXPECT(kinds[f] == w.kind && ij[2 * f] == w.i && ij[2 * f + 1] == w.j && huber[f] == w.huber);
    for (int c = 0; c < 6; ++c) EXPECT(sigmas[6 * f + static_cast<size_t>(c)] == w.sigma);
    EXPECT(std::memcmp(&data[16 * f], d.data(), sizeof(double) * 16) == 0);
  }
  EXPECT(fixed == (hold ? std::vector<uint8_t>({1, 1, 1, 0, 0}) : std::vector<uint8_t>({0, 0, 0, 0, 0})));
  char why[160] = "";
  std::vector<int32_t> off(6), inc(2 * kinds.size());
  EXPECT(smhip_pose_graph_plan_robust(5, poses.data(), fixed.data(), static_cast<int>(kinds.size()), kinds.data(), ij.data(), data.data(), sigmas.data(), huber.data(),
                                      off.data(), inc.data(), why, sizeof(why)) == SMHIP_OK);
  // nothing is solved before RunFinalOptimizing, and it is one solve
  EXPECT(opt.SolveCount() == 0 && g_host_solves == 0 && opt.LoopEdgeReport().empty());
  const std::vector<reg::Matrix4d> before = opt.Graph().Poses();
  EXPECT(opt.RunFinalOptimizing());
  EXPECT(opt.SolveCount() == 1 && g_host_solves == 1 && (g_host_stats.stop_reason == SMHIP_POSE_GRAPH_STOP_STEP || g_host_stats.stop_reason == SMHIP_POSE_GRAPH_STOP_COST));
  g_host_solves = 0;
  const std::vector<be::LoopEdgeWeight> rep = opt.LoopEdgeReport();
  EXPECT(rep.size() == 2 && rep[0].target == 1 && rep[0].source == 3 && rep[1].target == 2 && rep[1].source == 4 && rep[0].weight == 1.0 && rep[1].weight == 1.0);
  for (int k = 0; k < 3; ++k) {
    const bool same = std::memcmp(before[static_cast<size_t>(k)].data(), opt.Graph().Pose(k).data(), sizeof(double) * 16) == 0;
    EXPECT(same == hold);                                                                 // held: the base keeps its bits; free: it moves too
  }
  EXPECT(std::memcmp(before[3].data(), opt.Graph().Pose(3).data(), sizeof(double) * 16) != 0);
  EXPECT(std::memcmp(opt.GetLoopDetector()->GetFrames()[4]->global_pose.data(), opt.Graph().Pose(4).data(), sizeof(double) * 16) == 0);   // written back
  // the mutual pose at the submaps with a cross edge is the measured one (the two edges agree; the priors pull by sigma 0.1 against 0.025)
  for (int k = 0; k < 2; ++k) {
    const reg::Matrix4d m = be::Multiply(be::RigidInverse(opt.Graph().Pose(1 + k)), opt.Graph().Pose(3 + k)), z = CrossEdge(k);
    EXPECT(std::fabs(m(0, 3) - z(0, 3)) < 0.05 && std::fabs(m(1, 3) - z(1, 3)) < 0.05);
  }
}

static void ConnectionHuberIsAnOption() {
  be::MultiTrajectoryOptions o;
  o.connection_huber = 1.0; o.loop_closure_huber = 2.5;
  be::MultiTrajectoryOptimizer opt(o, be::LoopDetectorSettings(), nullptr);
  EXPECT(FeedThreeAndTwo(&opt));
  std::vector<double> huber;
  opt.Graph().FlattenHuber(&huber);
  EXPECT(huber == std::vector<double>({1.0, 1.0, 2.5, 2.5, 1.0, 0.0, 0.0}));
  bool threw = false;
  try { be::MultiTrajectoryOptions bad; bad.connection_huber = -1.0; be::MultiTrajectoryOptimizer x(bad, be::LoopDetectorSettings(), nullptr); } catch (const std::exception&) { threw = true; }
  EXPECT(threw);
}

static void Refusals() {
  be::MultiTrajectoryOptimizer opt(be::MultiTrajectoryOptions(), be::LoopDetectorSettings(), nullptr);
  EXPECT(opt.AddDetected(Frame(Pose(0, 0, 0, 0)), Id(0, 0), Detected(0, {})));
  EXPECT(opt.AddDetected(Frame(Pose(4, 0, 0, 0)), Id(0, 1), Detected(1, {})));
  // a loop edge inside one trajectory: the reference's CHECK_NE
  EXPECT(!opt.AddDetected(Frame(Pose(8, 0, 0, 0)), Id(0, 2), Detected(2, {{0, Pose(8, 0, 0, 0)}})));
  EXPECT(opt.LastError().find("joins two submaps of one trajectory") != std::string::npos && opt.Graph().VertexCount() == 2 && opt.Graph().Edges().empty());
  EXPECT(!opt.AddSubmapConnection(Id(0, 0), Id(0, 1), Pose(4, 0, 0, 0), true) && opt.LastError().find("joins two submaps of one trajectory") != std::string::npos);
  EXPECT(opt.AddSubmapConnection(Id(0, 0), Id(0, 1), Pose(4, 0, 0, 0), false) && opt.LoopEdgeCount() == 0);
  // ids out of order, a connection to a submap that was never added
  EXPECT(!opt.AddDetected(Frame(Pose(8, 0, 0, 0)), Id(0, 3), Detected(2, {})) && opt.LastError().find("out of order") != std::string::npos);
  EXPECT(!opt.AddDetected(Frame(Pose(8, 0, 0, 0)), Id(2, 0), Detected(2, {})) && opt.LastError().find("out of order") != std::string::npos);
  EXPECT(!opt.AddDetected(Frame(Pose(8, 0, 0, 0)), Id(1, 1), Detected(2, {})));
  EXPECT(!opt.AddSubmapConnection(Id(0, 1), Id(1, 0), Pose(0, 0, 0, 0), true) && opt.LastError().find("was not added") != std::string::npos);
  EXPECT(opt.Graph().VertexCount() == 2 && opt.Graph().Edges().size() == 1);
  // more nodes than one device solve takes: refused by size, the message names both sizes
  be::MultiTrajectoryOptimizer big(be::MultiTrajectoryOptions(), be::LoopDetectorSettings(), nullptr);
  bool ok = true;
  for (int k = 0; k < SMHIP_POSE_GRAPH_MAX_NODES && ok; ++k) ok = big.AddDetected(Frame(Pose(k, 0, 0, 0)), Id(0, k), Detected(k, {}));
  EXPECT(ok && big.Graph().NodeCount() == SMHIP_POSE_GRAPH_MAX_NODES);
  EXPECT(!big.AddDetected(Frame(Pose(-1, 0, 0, 0)), Id(1, 0), Detected(SMHIP_POSE_GRAPH_MAX_NODES, {})));
  EXPECT(big.LastError().find("would have 8193 nodes and 2 factors") != std::string::npos && big.LastError().find("at most 8192 nodes and 32768 factors") != std::string::npos);
  EXPECT(big.Graph().NodeCount() == SMHIP_POSE_GRAPH_MAX_NODES);
  // ... and more factors
  for (int round = 0; ok && big.Graph().FactorCount() < SMHIP_POSE_GRAPH_MAX_EDGES; ++round)
    for (int k = 0; k + 1 + round < SMHIP_POSE_GRAPH_MAX_NODES && big.Graph().FactorCount() < SMHIP_POSE_GRAPH_MAX_EDGES && ok; ++k)
      ok = big.AddSubmapConnection(Id(0, k), Id(0, k + 1 + round), Pose(1 + round, 0, 0, 0), false);
  EXPECT(ok && big.Graph().FactorCount() == SMHIP_POSE_GRAPH_MAX_EDGES);
  EXPECT(!big.AddSubmapConnection(Id(0, 0), Id(0, 5000), Pose(5000, 0, 0, 0), false));
  EXPECT(big.LastError().find("would have 8192 nodes and 32769 factors") != std::string::npos && big.Graph().FactorCount() == SMHIP_POSE_GRAPH_MAX_EDGES);
}

// the builder over the fixture, loaded as the base map and again as an incremental map: no device (ten submaps stay below the
// detector's loop_ignore_threshold, so no match is tried)
static void BuilderOffsets(const std::string& fixture, const std::string& tmp) {
  smhip::MultiTrajectoryMapBuilderOptions o;
  smhip::MultiTrajectoryMapBuilder b(o, nullptr);
  b.Optimizer()->SetSolver(HostSolve);
  EXPECT(!b.LoadIncrementalMap(fixture) && b.LastError().find("no base map") != std::string::npos);
  EXPECT(!b.LoadBaseMap(tmp + "/nowhere.xml") && b.LastError().find("map file does not exist") != std::string::npos);
  EXPECT(b.LoadBaseMap(fixture));
  EXPECT(b.BaseSubmapCount() == 5 && b.Map().trajectories.size() == 2 && b.Optimizer()->SolveCount() == 0);
  EXPECT(b.Optimizer()->GetLoopDetector()->SearchWindow() == std::make_pair(0, 4));
  // the connections of the file: (0,0)->(0,1), (0,1)->(0,2), (0,1)->(1,0), (1,0)->(1,1), each target^-1 source of the loaded poses
  const auto& edges = b.Optimizer()->Graph().Edges();
  EXPECT(edges.size() == 4 && edges[0].i == 0 && edges[0].j == 1 && edges[2].i == 1 && edges[2].j == 3 && edges[3].i == 3 && edges[3].j == 4);
  const reg::Matrix4d z = be::Multiply(be::RigidInverse(b.Map().trajectories[0].submaps[1].pose), b.Map().trajectories[1].submaps[0].pose);
  double worst = 0.0;
  for (int q = 0; q < 16 && edges.size() == 4; ++q) worst = std::fmax(worst, std::fabs(edges[2].transform.data()[q] - z.data()[q]));
  EXPECT(edges.size() == 4 && worst < 1e-14 && edges[2].huber == 0.0 && edges[2].sigmas[0] == 0.01);
  EXPECT(b.Optimizer()->Graph().Factors().size() == 2);                                   // a prior per trajectory
  // Loaded alone, the map is at its optimum.  On the device a forced solve starts at cost exactly 0 and moves no bit (ConnectionTransform;
  // tests/test_multi_trajectory_gpu.py); this CPU build of the kernel's loop does not contract its sums, so every entry of X_i^-1 X_j is
  // within 3 ulp of the measured one: a whitened residual below 1e-13 (sigma 0.01, poses within 12 m), a cost below 1e-24, poses within 1e-14.
  const std::vector<reg::Matrix4d> before = b.Optimizer()->Graph().Poses();
  EXPECT(b.Optimizer()->RunFinalOptimizing() && g_host_stats.initial_cost <= 1e-24 && g_host_stats.final_cost <= 1e-24);
  for (size_t k = 0; k < before.size(); ++k)
    for (int q = 0; q < 16; ++q) EXPECT(std::fabs(before[k].data()[q] - b.Optimizer()->Graph().Pose(static_cast<int>(k)).data()[q]) <= 1e-14);
  EXPECT(b.LoadIncrementalMap(fixture));
  EXPECT(b.IncrementalSubmapCount() == 5 && b.Map().trajectories.size() == 4 && b.Optimizer()->SolveCount() == 2 && b.Optimizer()->LoopEdgeCount() == 0);
  const auto& t = b.Map().trajectories;
  EXPECT(t[2].id == 2 && t[3].id == 3 && t[2].submaps[1].id == Id(2, 1) && t[3].submaps[0].id == Id(3, 0));
  EXPECT(t[2].submaps[1].connections == std::vector<bld::SubmapId>({Id(2, 2), Id(3, 0)}) && t[3].submaps[0].connections == std::vector<bld::SubmapId>({Id(3, 1)}));
  EXPECT(t[0].submaps[1].connections == std::vector<bld::SubmapId>({Id(0, 2), Id(1, 0)}));    // the base's own are as they were
  EXPECT(b.Optimizer()->Graph().Edges().size() == 8 && b.Optimizer()->Graph().Edges()[6].i == 6 && b.Optimizer()->Graph().Edges()[6].j == 8);
  EXPECT(b.Optimizer()->GetLoopDetector()->SearchWindow() == std::make_pair(0, 4));
  // the whole map, written beside the fixture's copy and read again
  EXPECT(b.SaveWholeMap(tmp + "/whole.xml"));
  bld::TrajectoryMap back;
  std::string why;
  EXPECT(bld::ReadTrajectoryMap(tmp + "/whole.xml", &back, &why) && back.trajectories.size() == 4 && back.SubmapCount() == 10);
  if (back.trajectories.size() == 4) {
    EXPECT(back.trajectories[2].submaps[1].connections == t[2].submaps[1].connections);
    for (size_t k = 0; k < 4; ++k)
      for (size_t s = 0; s < t[k].submaps.size(); ++s)
        EXPECT(std::memcmp(back.trajectories[k].submaps[s].pose.data(), t[k].submaps[s].pose.data(), sizeof(double) * 16) == 0 &&
               back.trajectories[k].submaps[s].Path() == t[k].submaps[s].Path());
  }
}

// ---- a join fed by hand ------------------------------------------------------------------------------------------------------------

// IN (text): hold_base loop_huber connection_huber; n_base n_inc; per submap 16 doubles (row-major), the base map's first; the number
// of cross edges; per cross edge base submap, incremental submap, 16 doubles (the incremental submap's pose in the base submap's
// frame).  The base map's submaps and connections (k, k + 1), UseCurrentStateAsBaseMap, the incremental map's submaps, each with the
// cross edges whose source it is as a detector result made by hand, its connections, RunFinalOptimizing.
static int Graph(const std::string& where, const char* path) {
  std::ifstream in(path);
  be::MultiTrajectoryOptions o;
  int hold = 0, nb = 0, ni = 0, nc = 0;
  if (!(in >> hold >> o.loop_closure_huber >> o.connection_huber >> nb >> ni)) return 2;
  o.hold_base_map = hold != 0;
  std::vector<reg::Matrix4d> pose(static_cast<size_t>(nb + ni));
  for (auto& m : pose) for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) in >> m(r, c);
  in >> nc;
  struct Cross { int b, s; reg::Matrix4d Z; };
  std::vector<Cross> cross(static_cast<size_t>(nc));
  for (auto& x : cross) { in >> x.b >> x.s; for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) in >> x.Z(r, c); }
  if (!in) return 2;
  std::shared_ptr<smhip::pre_processers::filter::DeviceContext> context;
  std::unique_ptr<be::MultiTrajectoryOptimizer> opt;
  if (where == "gpu") {
    context = smhip::pre_processers::filter::DeviceContext::Default();
    opt.reset(new be::MultiTrajectoryOptimizer(o, be::LoopDetectorSettings(), context->handle()));
  } else {
    opt.reset(new be::MultiTrajectoryOptimizer(o, be::LoopDetectorSettings(), nullptr));
    opt->SetSolver(HostSolve);
    opt->SetReporter(HostReport);
  }
  bool ok = true;
  for (int k = 0; k < nb; ++k) ok = opt->AddDetected(Frame(pose[static_cast<size_t>(k)]), Id(0, k), Detected(k, {})) && ok;
  for (int k = 0; k + 1 < nb; ++k)
    ok = opt->AddSubmapConnection(Id(0, k), Id(0, k + 1), be::Multiply(be::RigidInverse(pose[static_cast<size_t>(k)]), pose[static_cast<size_t>(k) + 1]), false) && ok;
  opt->UseCurrentStateAsBaseMap();
  for (int s = 0; s < ni; ++s) {
    std::vector<std::pair<int, reg::Matrix4d>> edges;
    for (const Cross& x : cross) if (x.s == s) edges.emplace_back(x.b, x.Z);
    ok = opt->AddDetected(Frame(pose[static_cast<size_t>(nb + s)]), Id(1, s), Detected(nb + s, edges)) && ok;
  }
  for (int s = 0; s + 1 < ni; ++s)
    ok = opt->AddSubmapConnection(Id(1, s), Id(1, s + 1), be::Multiply(be::RigidInverse(pose[static_cast<size_t>(nb + s)]), pose[static_cast<size_t>(nb + s) + 1]), false) && ok;
  const int solves_before = opt->SolveCount();
  ok = ok && opt->RunFinalOptimizing();
  if (!ok) std::fprintf(stderr, "%s\n", opt->LastError().c_str());
  const smhip_pose_graph_stats st = where == "gpu" ? opt->LastStats() : g_host_stats;
  const std::vector<be::LoopEdgeWeight> rep = opt->LoopEdgeReport();
  const auto window = opt->GetLoopDetector()->SearchWindow();
  std::printf("{\"ok\": %s, \"solves_before\": %d, \"solves\": %d, \"loop_edges\": %d, \"window\": [%d, %d], \"stop_reason\": %d, \"accepted_steps\": %d, \"rejected_steps\": %d, "
              "\"pcg_iterations\": %d, \"pcg_max_iterations\": %d, \"initial_cost\": %.17g, \"final_cost\": %.17g, \"damping\": %.17g, \"factors\": %d, \"report\": [",
              ok ? "true" : "false", solves_before, opt->SolveCount(), opt->LoopEdgeCount(), window.first, window.second, st.stop_reason, st.accepted_steps, st.rejected_steps,
              st.pcg_iterations, st.pcg_max_iterations, st.initial_cost, st.final_cost, st.damping, opt->Graph().FactorCount());
  for (size_t k = 0; k < rep.size(); ++k) std::printf("%s[%d, %d, %.17g, %.17g]", k ? ", " : "", rep[k].target, rep[k].source, rep[k].norm, rep[k].weight);
  std::printf("], \"fixed\": [");
  for (size_t k = 0; k < opt->Graph().Fixed().size(); ++k) std::printf("%s%d", k ? ", " : "", opt->Graph().Fixed()[k]);
  std::printf("], \"poses\": [");
  const auto& frames = opt->GetLoopDetector()->GetFrames();
  for (size_t k = 0; k < frames.size(); ++k) {
    std::printf("%s[", k ? ", " : "");
    for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) std::printf("%.17g%s", frames[k]->global_pose(r, q), (r == 3 && q == 3) ? "" : ", ");
    std::printf("]");
  }
  std::printf("]}\n");
  return 0;
}

// ---- the builder on map files ------------------------------------------------------------------------------------------------------

static void PrintMap(const smhip::MultiTrajectoryMapBuilder& b) {
  std::printf("\"trajectories\": [");
  for (size_t t = 0; t < b.Map().trajectories.size(); ++t) {
    std::printf("%s[", t ? ", " : "");
    const auto& subs = b.Map().trajectories[t].submaps;
    for (size_t s = 0; s < subs.size(); ++s) {
      std::printf("%s{\"connections\": \"%s\", \"pose\": [", s ? ", " : "", bld::ConnectionsIdsToStr(subs[s].connections).c_str());
      for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) std::printf("%.17g%s", subs[s].pose(r, q), (r == 3 && q == 3) ? "" : ", ");
      std::printf("]}");
    }
    std::printf("]");
  }
  std::printf("]");
}

static int Base(const std::string& where, const char* map_xml) {
  std::shared_ptr<smhip::pre_processers::filter::DeviceContext> context;
  if (where == "gpu") context = smhip::pre_processers::filter::DeviceContext::Default();
  smhip::MultiTrajectoryMapBuilderOptions o;
  smhip::MultiTrajectoryMapBuilder b(o, context ? context->handle() : nullptr);
  if (!context) b.Optimizer()->SetSolver(HostSolve);
  if (!b.LoadBaseMap(map_xml)) { std::printf("{\"ok\": false, \"why\": \"%s\"}\n", b.LastError().c_str()); return 0; }
  const std::vector<reg::Matrix4d> before = b.Optimizer()->Graph().Poses();
  const bool ok = b.Optimizer()->RunFinalOptimizing();
  bool moved = false;
  for (size_t k = 0; k < before.size(); ++k) {
    moved = moved || std::memcmp(before[k].data(), b.Optimizer()->Graph().Pose(static_cast<int>(k)).data(), sizeof(double) * 16) != 0;
    moved = moved || std::memcmp(before[k].data(), b.Optimizer()->GetLoopDetector()->GetFrames()[k]->global_pose.data(), sizeof(double) * 16) != 0;
    for (int q = 0; q < 16; ++q) {                                      // (which entry, for the reader of a failure)
      const double was = before[k].data()[q], is = b.Optimizer()->Graph().Pose(static_cast<int>(k)).data()[q];
      if (std::memcmp(&was, &is, sizeof(double)) != 0) std::fprintf(stderr, "node %zu entry %d (column-major): %a -> %a\n", k, q, was, is);
    }
  }
  const smhip_pose_graph_stats st = context ? b.Optimizer()->LastStats() : g_host_stats;
  std::printf("{\"ok\": %s, \"submaps\": %d, \"factors\": %d, \"solves\": %d, \"initial_cost\": %.17g, \"final_cost\": %.17g, \"stop_reason\": %d, \"a_bit_moved\": %s}\n",
              ok ? "true" : "false", b.BaseSubmapCount(), b.Optimizer()->Graph().FactorCount(), b.Optimizer()->SolveCount(), st.initial_cost, st.final_cost, st.stop_reason,
              moved ? "true" : "false");
  return 0;
}

static int Join(int argc, char** argv) {
  // join gpu BASE INC OUT HOLD M2DP_SCORE [PCD STATIC]
  auto context = smhip::pre_processers::filter::DeviceContext::Default();
  smhip::MultiTrajectoryMapBuilderOptions o;
  o.optimizer.hold_base_map = std::atoi(argv[6]) != 0;
  o.loop_detect_settings.use_descriptor = true;                                           // every loaded submap's descriptor comes from the device
  o.loop_detect_settings.m2dp_match_score = static_cast<float>(std::atof(argv[7]));
  o.loop_detect_settings.loop_ignore_threshold = 2;                                       // (the maps of the test have six submaps each)
  o.loop_detect_settings.max_close_loop_distance = 6.f;                                   // the submap at the same place and its neighbours
  o.max_clouds_in_memory = 4;                                                             // fewer than the twelve submaps: clouds are loaded again
  smhip::MultiTrajectoryMapBuilder b(o, context->handle());
  if (!b.LoadBaseMap(argv[3]) || !b.LoadIncrementalMap(argv[4]) || !b.SaveWholeMap(argv[5])) { std::printf("{\"ok\": false, \"why\": \"%s\"}\n", b.LastError().c_str()); return 0; }
  bool ok = true;
  if (argc == 10) ok = b.GenerateWholeMapPcd(argv[8]) && b.GenerateStaticMap(argv[9]);
  if (!ok) { std::printf("{\"ok\": false, \"why\": \"%s\"}\n", b.LastError().c_str()); return 0; }
  const smhip_pose_graph_stats st = b.Optimizer()->LastStats();
  std::printf("{\"ok\": true, \"base_submaps\": %d, \"incremental_submaps\": %d, \"loop_edges\": %d, \"solves\": %d, \"stop_reason\": %d, \"pcg_iterations\": %d, "
              "\"pcg_max_iterations\": %d, \"clouds_in_memory\": %d, \"cloud_loads\": %lld, \"whole_map_points\": %lld, \"static_map_voxels\": %d, \"edges\": [",
              b.BaseSubmapCount(), b.IncrementalSubmapCount(), b.Optimizer()->LoopEdgeCount(), b.Optimizer()->SolveCount(), st.stop_reason, st.pcg_iterations,
              st.pcg_max_iterations, b.CloudsInMemory(), b.CloudLoads(), b.WholeMapPoints(), b.StaticMapVoxels());
  const std::vector<be::LoopEdgeWeight> rep = b.Optimizer()->LoopEdgeReport();
  for (size_t k = 0; k < rep.size(); ++k) {
    const bld::SubmapId t = b.Optimizer()->IdOf(rep[k].target), s = b.Optimizer()->IdOf(rep[k].source);
    std::printf("%s[%d, %d, %d, %d, %.17g, %.17g]", k ? ", " : "", t.trajectory_index, t.submap_index, s.trajectory_index, s.submap_index, rep[k].norm, rep[k].weight);
  }
  std::printf("], ");
  PrintMap(b);
  std::printf("}\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "host" && argc == 4) {
    FactorList(false);
    FactorList(true);
    ConnectionHuberIsAnOption();
    Refusals();
    BuilderOffsets(argv[2], argv[3]);
    std::printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
  }
  if (mode == "graph" && argc == 4) return Graph(argv[2], argv[3]);
  if (mode == "base" && argc == 4) return Base(argv[2], argv[3]);
  if (mode == "join" && (argc == 8 || argc == 10) && std::string(argv[2]) == "gpu") return Join(argc, argv);
  std::fprintf(stderr, "usage: test_multi_trajectory host FIXTURE TMPDIR | graph host|gpu IN | base host|gpu MAP | join gpu BASE INC OUT HOLD M2DP_SCORE [PCD STATIC]\n");
  return 2;
}
