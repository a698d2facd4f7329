// The pose-graph optimiser: include/smhip/pose_graph.h, the host half of smhip_pose_graph_optimize (csrc/pose_graph_plan.h) and the
// kernel's loop compiled for the CPU (csrc/pose_graph_kernel.h with HostCtx: one thread, empty barriers).
//   test_pose_graph host               no device: every refusal, the CSR order, Submap::UpdateInnerFramePose, IsamOptimizer's
//                                      bookkeeping on hand-made detector results (solved by the kernel's loop on the CPU)
//   test_pose_graph solve IN OUT       the kernel's loop on the CPU for the problem in IN (see ReadProblem), results to OUT
//   test_pose_graph gpu <dir> <scans> <frame_count> <m2dp_match_score>
//                                      <dir>/NNNNNN.bin scans, <dir>/poses.txt the poses fed to the back end (16 doubles per line,
//                                      row-major): submaps, descriptors, IsamOptimizer::AddFrame per submap on the device; one
//                                      JSON line with every submap's pose afterwards
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
using smhip::data::InnerCloudType;
using smhip::data::InnerPointType;

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
  std::vector<int32_t> fixed, ij, csr_off, csr_edge;
  std::vector<double> work, out_d;
  std::vector<int32_t> out_i;
  pg::Dev d;

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
    d.fixed = fixed.data(); d.ij = ij.data(); d.csr_off = csr_off.data(); d.csr_edge = csr_edge.data();
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

// IsamOptimizer's solver without a device: smhip_pose_graph_optimize's host half, then the kernel's loop on this thread
static bool HostSolve(be::PoseGraph* graph) {
  std::vector<double> poses, Z, sigmas;
  std::vector<int32_t> ij;
  graph->Flatten(&poses, &ij, &Z, &sigmas);
  HostProblem hp;
  hp.n = graph->VertexCount(); hp.m = static_cast<int>(graph->Edges().size());
  pg::Plan plan;
  std::string why;
  if (pg::check_and_plan(hp.n, poses.data(), graph->Fixed().data(), hp.m, ij.data(), Z.data(), sigmas.data(), &plan, &why) != SMHIP_OK) {
    std::fprintf(stderr, "%s\n", why.c_str());
    return false;
  }
  hp.pose0.resize(12 * static_cast<size_t>(hp.n)); hp.Z.resize(12 * static_cast<size_t>(hp.m)); hp.sinv.resize(6 * static_cast<size_t>(hp.m));
  for (int k = 0; k < hp.n; ++k) Pack12(&poses[16 * static_cast<size_t>(k)], &hp.pose0[12 * static_cast<size_t>(k)]);
  for (int e = 0; e < hp.m; ++e) Pack12(&Z[16 * static_cast<size_t>(e)], &hp.Z[12 * static_cast<size_t>(e)]);
  for (size_t k = 0; k < sigmas.size(); ++k) hp.sinv[k] = 1.0 / sigmas[k];
  hp.fixed.assign(graph->Fixed().begin(), graph->Fixed().end());
  hp.ij = ij; hp.csr_off = plan.csr_offsets; hp.csr_edge = plan.csr_edges;
  hp.Bind(50, plan.pcg_cap);
  pg::HostCtx c;
  pg::run(hp.d, c);
  if (hp.out_i[pg::kOutStop] == SMHIP_POSE_GRAPH_STOP_NUMERIC) return false;
  for (int k = 0; k < hp.n; ++k) {
    if (hp.fixed[static_cast<size_t>(k)]) continue;
    const double* p = hp.d.cur + 12 * static_cast<size_t>(k);
    double* o = &poses[16 * static_cast<size_t>(k)];
    for (int r = 0; r < 3; ++r) { for (int q = 0; q < 3; ++q) o[4 * q + r] = p[3 * r + q]; o[12 + r] = p[9 + r]; }
  }
  graph->SetFlatPoses(poses);
  return true;
}

// IN: int32 n, m; then doubles pose0[12 n], Z[12 m], sinv[6 m], v[6 n]; then int32 fixed[n], ij[2 m], max_it.  OUT: doubles cur[12 n],
// out_d[3], out_i[6] (as doubles), then of a second, probing run: rw[6 m], A[36 m], B[36 m], g[6 n], minv[6 n].
static int Solve(const char* in_path, const char* out_path) {
  std::ifstream in(in_path, std::ios::binary);
  HostProblem hp;
  int32_t nm[2];
  if (!in.read(reinterpret_cast<char*>(nm), sizeof(nm))) return 2;
  hp.n = nm[0]; hp.m = nm[1];
  const size_t N = static_cast<size_t>(hp.n), M = static_cast<size_t>(hp.m);
  hp.pose0.resize(12 * N); hp.Z.resize(12 * M); hp.sinv.resize(6 * M); hp.v.resize(6 * N); hp.fixed.resize(N); hp.ij.resize(2 * M);
  int32_t max_it = 0;
  auto rd = [&in](void* p, size_t bytes) { return bytes == 0 || static_cast<bool>(in.read(reinterpret_cast<char*>(p), static_cast<std::streamsize>(bytes))); };
  if (!rd(hp.pose0.data(), 96 * N) || !rd(hp.Z.data(), 96 * M) || !rd(hp.sinv.data(), 48 * M) || !rd(hp.v.data(), 48 * N) || !rd(hp.fixed.data(), 4 * N) ||
      !rd(hp.ij.data(), 8 * M) || !rd(&max_it, 4))
    return 2;
  // the CSR list as the library makes it (the checks want 4x4 column-major input: build the list alone here)
  hp.csr_off.assign(N + 1, 0);
  for (size_t e = 0; e < M; ++e) { ++hp.csr_off[static_cast<size_t>(hp.ij[2 * e]) + 1]; ++hp.csr_off[static_cast<size_t>(hp.ij[2 * e + 1]) + 1]; }
  for (size_t k = 0; k < N; ++k) hp.csr_off[k + 1] += hp.csr_off[k];
  hp.csr_edge.assign(2 * M, 0);
  std::vector<int32_t> at(hp.csr_off.begin(), hp.csr_off.end() - 1);
  int non_chain = 0;
  for (size_t e = 0; e < M; ++e) {
    hp.csr_edge[static_cast<size_t>(at[static_cast<size_t>(hp.ij[2 * e])]++)] = static_cast<int32_t>(e);
    hp.csr_edge[static_cast<size_t>(at[static_cast<size_t>(hp.ij[2 * e + 1])]++)] = static_cast<int32_t>(e);
    if (std::abs(hp.ij[2 * e] - hp.ij[2 * e + 1]) != 1) ++non_chain;
  }
  hp.Bind(max_it, 12 * non_chain + 64);
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

struct Graph {                       // a chain 0 - 1 - 2 - 3 with one loop edge (0, 3), node 0 fixed: accepted as it stands
  std::vector<double> poses, Z, sigmas;
  std::vector<uint8_t> fixed;
  std::vector<int32_t> ij;
  Graph() {
    for (int k = 0; k < 4; ++k) { const reg::Matrix4d p = Pose(k, 0.1 * k, 0, 0.2 * k); poses.insert(poses.end(), p.m, p.m + 16); fixed.push_back(k == 0); }
    const int e[4][2] = {{0, 1}, {1, 2}, {2, 3}, {0, 3}};
    for (const auto& p : e) {
      ij.push_back(p[0]); ij.push_back(p[1]);
      const reg::Matrix4d z = Pose(p[1] - p[0], 0, 0, 0.1);
      Z.insert(Z.end(), z.m, z.m + 16);
      for (int c = 0; c < 6; ++c) sigmas.push_back(c < 3 ? 0.1 : 0.15);
    }
  }
  smhip_status Check(std::string* why = nullptr, pg::Plan* plan = nullptr) const {
    return pg::check_and_plan(static_cast<int>(fixed.size()), poses.data(), fixed.data(), static_cast<int>(ij.size() / 2), ij.data(), Z.data(),
                              sigmas.empty() ? nullptr : sigmas.data(), plan, why);
  }
  // the same through the library's symbol, which needs no device
  smhip_status CheckAbi() const {
    char why[256];
    return smhip_pose_graph_plan(static_cast<int>(fixed.size()), poses.data(), fixed.data(), static_cast<int>(ij.size() / 2), ij.data(), Z.data(),
                                 sigmas.empty() ? nullptr : sigmas.data(), nullptr, nullptr, why, sizeof(why));
  }
};

static void RefusalChecks() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  auto refused = [](const Graph& g, smhip_status want) {
    std::string why;
    const smhip_status a = g.Check(&why), b = g.CheckAbi();
    if (a != want || b != want || why.empty()) std::fprintf(stderr, "  got %d / %d (%s), want %d\n", a, b, why.c_str(), want);
    return a == want && b == want && !why.empty();
  };
  { Graph g; EXPECT(g.Check() == SMHIP_OK && g.CheckAbi() == SMHIP_OK); }
  { Graph g; g.sigmas.clear(); EXPECT(g.Check() == SMHIP_OK); }                                  // null sigmas = the defaults
  { Graph g; EXPECT(pg::check_and_plan(4, nullptr, g.fixed.data(), 4, g.ij.data(), g.Z.data(), nullptr, nullptr, nullptr) == SMHIP_ERR_INVALID_ARGUMENT); }
  { Graph g; EXPECT(pg::check_and_plan(4, g.poses.data(), nullptr, 4, g.ij.data(), g.Z.data(), nullptr, nullptr, nullptr) == SMHIP_ERR_INVALID_ARGUMENT); }
  { Graph g; EXPECT(pg::check_and_plan(4, g.poses.data(), g.fixed.data(), 4, nullptr, g.Z.data(), nullptr, nullptr, nullptr) == SMHIP_ERR_INVALID_ARGUMENT); }
  { Graph g; EXPECT(pg::check_and_plan(4, g.poses.data(), g.fixed.data(), 4, g.ij.data(), nullptr, nullptr, nullptr, nullptr) == SMHIP_ERR_INVALID_ARGUMENT); }
  { Graph g; EXPECT(pg::check_and_plan(0, g.poses.data(), g.fixed.data(), 0, g.ij.data(), g.Z.data(), nullptr, nullptr, nullptr) == SMHIP_ERR_INVALID_ARGUMENT); }
  { Graph g; g.ij[3] = 4; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }                      // an index out of range
  { Graph g; g.ij[2] = -1; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }
  { Graph g; g.ij[6] = 3; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }                      // i == j
  { Graph g; g.sigmas[7] = 0.0; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }
  { Graph g; g.sigmas[7] = -0.1; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }
  { Graph g; g.sigmas[0] = nan; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }
  { Graph g; g.sigmas[23] = inf; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }
  { Graph g; g.poses[16 + 12] = nan; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }           // a non-finite pose
  { Graph g; g.Z[32 + 13] = inf; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }               // a non-finite Z
  { Graph g; g.poses[32] += 2.0e-6; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }            // a rotation 2e-6 from orthonormal
  { Graph g; g.poses[32] += 2.0e-7; EXPECT(g.Check() == SMHIP_OK); }                             // 2e-7 (4e-7 in the column's norm) passes
  { Graph g; g.Z[16 + 5] *= 1.0 + 4.0e-6; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }
  { Graph g; for (int r = 0; r < 3; ++r) g.poses[48 + 8 + r] = -g.poses[48 + 8 + r]; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }   // a reflection
  {   // a free node without an edge
    Graph g;
    const reg::Matrix4d p = Pose(9, 9, 0, 0);
    g.poses.insert(g.poses.end(), p.m, p.m + 16); g.fixed.push_back(0);
    EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT));
    g.fixed.back() = 1;                                                                          // fixed, it needs none
    EXPECT(g.Check() == SMHIP_OK);
  }
  {   // a component without a fixed node: 4 - 5 joined to each other only
    Graph g;
    for (int k = 4; k < 6; ++k) { const reg::Matrix4d p = Pose(k, 0, 0, 0); g.poses.insert(g.poses.end(), p.m, p.m + 16); g.fixed.push_back(0); }
    g.ij.push_back(4); g.ij.push_back(5);
    const reg::Matrix4d z = Pose(1, 0, 0, 0);
    g.Z.insert(g.Z.end(), z.m, z.m + 16);
    for (int c = 0; c < 6; ++c) g.sigmas.push_back(0.1);
    EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT));
    g.fixed[5] = 1;
    EXPECT(g.Check() == SMHIP_OK);
  }
  { Graph g; g.fixed[0] = 0; EXPECT(refused(g, SMHIP_ERR_INVALID_ARGUMENT)); }                   // no fixed node at all
  {   // the limits: decided from the sizes alone (the arrays here are far shorter than the sizes claim)
    Graph g;
    EXPECT(pg::check_and_plan(pg::kMaxNodes + 1, g.poses.data(), g.fixed.data(), 4, g.ij.data(), g.Z.data(), nullptr, nullptr, nullptr) == SMHIP_ERR_CAPACITY);
    EXPECT(pg::check_and_plan(4, g.poses.data(), g.fixed.data(), pg::kMaxEdges + 1, g.ij.data(), g.Z.data(), nullptr, nullptr, nullptr) == SMHIP_ERR_CAPACITY);
    char why[64];
    EXPECT(smhip_pose_graph_plan(pg::kMaxNodes + 1, g.poses.data(), g.fixed.data(), 4, g.ij.data(), g.Z.data(), nullptr, nullptr, nullptr, why, sizeof(why)) == SMHIP_ERR_CAPACITY);
    EXPECT(std::strstr(why, "8192") != nullptr);
    // a null handle is refused before anything else
    EXPECT(smhip_pose_graph_optimize(nullptr, 4, g.poses.data(), g.fixed.data(), 4, g.ij.data(), g.Z.data(), nullptr, nullptr, nullptr) == SMHIP_ERR_INVALID_ARGUMENT);
  }
  {   // exactly at the limits: accepted.  A chain of kMaxNodes nodes, and edges up to kMaxEdges by repeating loop edges (0, k)
    const int n = pg::kMaxNodes, m = pg::kMaxEdges;
    std::vector<double> poses(16 * static_cast<size_t>(n)), Z(16 * static_cast<size_t>(m));
    std::vector<uint8_t> fixed(static_cast<size_t>(n), 0);
    std::vector<int32_t> ij(2 * static_cast<size_t>(m));
    const reg::Matrix4d I = reg::Matrix4d::Identity();
    for (int k = 0; k < n; ++k) std::memcpy(&poses[16 * static_cast<size_t>(k)], I.m, sizeof(I.m));
    for (int e = 0; e < m; ++e) {
      std::memcpy(&Z[16 * static_cast<size_t>(e)], I.m, sizeof(I.m));
      ij[2 * static_cast<size_t>(e)] = e < n - 1 ? e : 0;
      ij[2 * static_cast<size_t>(e) + 1] = e < n - 1 ? e + 1 : 2 + e % (n - 2);
    }
    fixed[0] = 1;
    pg::Plan plan;
    EXPECT(pg::check_and_plan(n, poses.data(), fixed.data(), m, ij.data(), Z.data(), nullptr, &plan, nullptr) == SMHIP_OK);
    EXPECT(plan.levels == 13 && plan.non_chain_edges == m - (n - 1) && plan.pcg_cap == 12 * (m - (n - 1)) + 64);
    EXPECT(plan.csr_offsets.back() == 2 * m);
  }
}

static void CsrChecks() {
  Graph g;
  // edges: 0 (0,1)  1 (1,2)  2 (2,3)  3 (0,3); add 4 (3,1) and 5 (1,0): a reversed chain edge counts as a chain edge
  const int extra[2][2] = {{3, 1}, {1, 0}};
  for (const auto& p : extra) {
    g.ij.push_back(p[0]); g.ij.push_back(p[1]);
    const reg::Matrix4d z = Pose(0, 0, 0, 0);
    g.Z.insert(g.Z.end(), z.m, z.m + 16);
    for (int c = 0; c < 6; ++c) g.sigmas.push_back(0.2);
  }
  pg::Plan plan;
  EXPECT(g.Check(nullptr, &plan) == SMHIP_OK);
  EXPECT(plan.csr_offsets == std::vector<int32_t>({0, 3, 7, 9, 12}));
  EXPECT(plan.csr_edges == std::vector<int32_t>({0, 3, 5, 0, 1, 4, 5, 1, 2, 2, 3, 4}));          // ascending within every node
  EXPECT(plan.non_chain_edges == 2 && plan.pcg_cap == 88 && plan.levels == 2);
  std::vector<int32_t> off(5), edges(12);
  char why[8];
  EXPECT(smhip_pose_graph_plan(4, g.poses.data(), g.fixed.data(), 6, g.ij.data(), g.Z.data(), g.sigmas.data(), off.data(), edges.data(), why, sizeof(why)) == SMHIP_OK);
  EXPECT(off == plan.csr_offsets && edges == plan.csr_edges && why[0] == '\0');
  smhip_pose_graph_options o;
  smhip_pose_graph_default_options(&o);
  EXPECT(o.max_iterations == 50);
}

static double Distance(const reg::Matrix4d& a, const reg::Matrix4d& b) {
  double s = 0;
  for (int q = 0; q < 16; ++q) s = std::fmax(s, std::fabs(a.m[q] - b.m[q]));
  return s;
}

static void UpdateInnerFramePoseChecks() {
  bld::SubmapOptions opt;
  opt.frame_count = 3;
  bld::Submap s(opt);
  InnerCloudType::Ptr cloud(new InnerCloudType);
  const reg::Matrix4d p0 = Pose(1, 2, 0.5, 0.3), p1 = Pose(2, 2.5, 0.5, 0.35), p2 = Pose(3, 3.1, 0.6, 0.4);
  s.InsertFrame(cloud, p0); s.InsertFrame(cloud, p1); s.InsertFrame(cloud, p2);
  EXPECT(Distance(s.GlobalPose(), p0) == 0.0 && Distance(s.FrameGlobalPose(2), p2) == 0.0);
  s.UpdateInnerFramePose();                                                                      // nothing moved: the same poses up to rounding
  EXPECT(Distance(s.FrameGlobalPose(1), p1) < 1e-15 && Distance(s.FrameGlobalPose(2), p2) < 1e-15);
  const reg::Matrix4d moved = Pose(-4, 7, 1, 1.2);
  s.SetGlobalPose(moved);
  EXPECT(Distance(s.FrameGlobalPose(1), p1) < 1e-15);                                            // not before the call
  s.UpdateInnerFramePose();
  EXPECT(Distance(s.FrameGlobalPose(0), moved) == 0.0);
  for (int k = 1; k < 3; ++k) EXPECT(Distance(s.FrameGlobalPose(k), be::Multiply(moved, s.LocalPose(k))) == 0.0);
  EXPECT(Distance(s.FirstFramePose(), moved) == 0.0);
}

static void IsamOptimizerChecks() {
  // five submaps on a square-ish drive that returns to its start; the fed poses drift by 0.4 m in y from the third on
  const reg::Matrix4d truth[5] = {Pose(0, 0, 0, 0), Pose(5, 0, 0, 0.8), Pose(8, 4, 0, 1.9), Pose(4, 7, 0, 3.1), Pose(0.5, 0.2, 0, 0.05)};
  be::LoopDetectorSettings lds;                      // loop_ignore_threshold 15: the detector itself never searches here
  be::IsamOptimizer opt(be::IsamOptimizerOptions(), lds, nullptr);
  opt.SetSolver(HostSolve);
  std::vector<std::shared_ptr<be::LoopFrame>> frames;
  for (int k = 0; k < 5; ++k) {
    std::shared_ptr<be::LoopFrame> f(new be::LoopFrame);
    f->global_pose = truth[k];
    if (k >= 2) f->global_pose(1, 3) += 0.4;
    frames.push_back(f);
  }
  auto odom = [&](int k) { return k == 0 ? reg::Matrix4d::Identity() : be::Multiply(be::RigidInverse(frames[k - 1]->global_pose), frames[k]->global_pose); };
  std::vector<reg::Matrix4d> odoms;
  for (int k = 0; k < 5; ++k) odoms.push_back(odom(k));                                          // (before anything is written back)
  for (int k = 0; k < 4; ++k) {
    be::DetectResult r;
    r.current_frame_index = k;
    if (k == 3) {                                                                                // edges without close_succeed add nothing (:227)
      be::LoopEdge e;
      e.close_pair_index = {0, 3};
      r.edges.push_back(e);
    }
    const reg::Matrix4d fed = frames[k]->global_pose;
    opt.AddDetected(frames[k], odoms[k], r);
    EXPECT(opt.Graph().VertexCount() == k + 1 && static_cast<int>(opt.Graph().Edges().size()) == k && opt.LoopEdgeCount() == 0);
    EXPECT(Distance(frames[k]->global_pose, fed) < 1e-9);                                         // a consistent chain stays where it is
  }
  EXPECT(opt.SolveCount() == 3);                                                                 // none for the first vertex
  EXPECT(opt.Graph().Fixed() == std::vector<uint8_t>({1, 0, 0, 0}));
  be::DetectResult wrong;
  wrong.current_frame_index = 7;
  bool threw = false;
  try { opt.AddDetected(frames[4], odoms[4], wrong); } catch (const std::exception&) { threw = true; }
  EXPECT(threw && opt.Graph().VertexCount() == 4);                                               // CHECK_EQ(frame_index, result.current_frame_index)
  be::DetectResult loop;
  loop.current_frame_index = 4;
  loop.close_succeed = true;
  for (int target = 0; target < 2; ++target) {
    be::LoopEdge e;
    e.close_pair_index = {target, 4};
    e.transform = be::Multiply(be::RigidInverse(truth[target]), truth[4]);
    loop.edges.push_back(e);
  }
  const double before = std::fabs(frames[4]->global_pose(1, 3) - truth[4](1, 3));
  opt.AddDetected(frames[4], odoms[4], loop);
  EXPECT(opt.LoopEdgeCount() == 2 && opt.Graph().Edges().size() == 6 && opt.SolveCount() == 5);
  EXPECT(opt.Graph().Edges()[4].i == 0 && opt.Graph().Edges()[4].j == 4 && opt.Graph().Edges()[5].i == 1);
  // every frame was written back, the first is where it was, and the last moved towards the truth
  for (int k = 0; k < 5; ++k) EXPECT(Distance(frames[k]->global_pose, opt.Graph().Pose(k)) == 0.0);
  EXPECT(Distance(frames[0]->global_pose, truth[0]) == 0.0);
  const double after = std::fabs(frames[4]->global_pose(1, 3) - truth[4](1, 3));
  EXPECT(before > 0.39 && after < 0.5 * before);
  const auto whole = opt.GetWholeGraph();
  EXPECT(whole.size() == 5 && whole[0].connections.size() == 2 && whole[0].connections[1].first == 4 && whole[1].connections.size() == 2 &&
         whole[4].connections.empty() && Distance(whole[3].pose, frames[3]->global_pose) == 0.0);
  const reg::Matrix4d last = frames[4]->global_pose;
  opt.RunFinalOptimazation();
  EXPECT(opt.SolveCount() == 6 && Distance(frames[4]->global_pose, last) < 1e-9);                // already at the minimum
}

// ---- the device --------------------------------------------------------------------------------------------------------------

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
  const auto context = smhip::pre_processers::filter::DeviceContext::Default();
  be::IsamOptimizer optimizer(be::IsamOptimizerOptions(), s, context->handle());
  std::vector<std::shared_ptr<be::LoopFrame>> frames;
  std::printf("{\"status\": [");
  for (size_t k = 0; k < maps.size(); ++k) {
    std::shared_ptr<be::LoopFrame> f(new be::LoopFrame);
    f->global_pose = maps[k]->GlobalPose();
    if (!maps[k]->CalculateDescriptor()) return 3;
    f->descriptor = maps[k]->GetDescriptor();
    f->cloud = maps[k]->Cloud();
    // the odometry factor: the fed poses' own step (the drift sits in one of them)
    const reg::Matrix4d from_last = k == 0 ? reg::Matrix4d::Identity() : be::Multiply(be::RigidInverse(maps[k - 1]->FirstFramePose()), maps[k]->FirstFramePose());
    frames.push_back(f);
    optimizer.AddFrame(f, from_last);
    std::printf("%s%d", k ? ", " : "", static_cast<int>(optimizer.GetLoopDetector()->Status()));
  }
  optimizer.RunFinalOptimazation();
  const smhip_pose_graph_stats& st = optimizer.LastStats();
  std::printf("], \"loop_edges\": %d, \"solves\": %d, \"stop_reason\": %d, \"final_cost\": %.17g, \"poses\": [", optimizer.LoopEdgeCount(), optimizer.SolveCount(),
              st.stop_reason, st.final_cost);
  for (size_t k = 0; k < maps.size(); ++k) {
    maps[k]->SetGlobalPose(frames[k]->global_pose);
    maps[k]->UpdateInnerFramePose();
    std::printf("%s[", k ? ", " : "");
    for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) std::printf("%.17g%s", frames[k]->global_pose(r, q), (r == 3 && q == 3) ? "" : ", ");
    std::printf("]");
  }
  std::printf("], \"last_frame_poses\": [");
  for (int i = 0; i < frame_count; ++i) {
    std::printf("%s[", i ? ", " : "");
    for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) std::printf("%.17g%s", maps.back()->FrameGlobalPose(i)(r, q), (r == 3 && q == 3) ? "" : ", ");
    std::printf("]");
  }
  std::printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "host") {
    RefusalChecks();
    CsrChecks();
    UpdateInnerFramePoseChecks();
    IsamOptimizerChecks();
    std::printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
  }
  if (mode == "solve" && argc == 4) return Solve(argv[2], argv[3]);
  if (mode == "gpu") return Gpu(argc, argv);
  std::fprintf(stderr, "usage: test_pose_graph host | solve IN OUT | gpu <dir> <scans> <frame_count> <m2dp_match_score>\n");
  return 2;
}
