// IsamOptimizer's marginal-covariance calls (include/smhip/pose_graph.h) on the host, with SetSolver and SetMarginalizer standing in for
// the device: what is refused before a solve, which nodes are asked for, and how the 12x12 joint is put together from two queries.
#define SMHIP_REGISTRATOR_THROW_ON_CHECK 1
#include <cstdio>
#include <memory>
#include <vector>

#include "smhip/pose_graph.h"

namespace be = smhip::back_end;
namespace reg = smhip::registrator;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
  be::LoopDetectorSettings lds;
  be::IsamOptimizerOptions io;
  io.use_odom = true; io.odom_extrinsic_calib = true;
  be::IsamOptimizer opt(io, lds, nullptr);
  std::vector<std::vector<int>> asked, asked_rows;
  opt.SetSolver([](be::PoseGraph*) { return true; });
  // cov[q] = 100 node + entry; blocks[q R + r] = 1000 row + 10 node + entry / 100: [H^-1]_{row, node}
  opt.SetMarginalizer([&](const be::PoseGraph&, const std::vector<int>& nodes, std::vector<std::array<double, 36>>* cov, const std::vector<int>* rows,
                          std::vector<std::array<double, 36>>* blocks) {
    asked.push_back(nodes);
    asked_rows.push_back(rows ? *rows : std::vector<int>());
    cov->assign(nodes.size(), std::array<double, 36>{});
    for (size_t q = 0; q < nodes.size(); ++q) for (int a = 0; a < 36; ++a) (*cov)[q][static_cast<size_t>(a)] = 100.0 * nodes[q] + a;
    if (blocks) {
      blocks->assign(nodes.size() * rows->size(), std::array<double, 36>{});
      for (size_t q = 0; q < nodes.size(); ++q)
        for (size_t r = 0; r < rows->size(); ++r)
          for (int a = 0; a < 36; ++a) (*blocks)[q * rows->size() + r][static_cast<size_t>(a)] = 1000.0 * (*rows)[r] + 10.0 * nodes[q] + a / 100.0;
    }
    return true;
  });
  std::array<double, 36> cov{};
  std::array<double, 144> joint{};
  EXPECT(!opt.MarginalCovariance(0, &cov) && asked.empty());                     // no vertex, no solve
  std::vector<std::shared_ptr<be::LoopFrame>> frames;
  for (int k = 0; k < 3; ++k) {
    std::shared_ptr<be::LoopFrame> f(new be::LoopFrame);
    f->global_pose = reg::Matrix4d::Identity();
    f->global_pose(0, 3) = k;
    frames.push_back(f);
    be::DetectResult r;
    r.current_frame_index = k;
    reg::Matrix4d step = reg::Matrix4d::Identity();
    step(0, 3) = k ? 1.0 : 0.0;
    EXPECT(opt.AddDetected(f, step, r));
    if (k == 0) EXPECT(!opt.MarginalCovariance(0, &cov) && asked.empty());       // one vertex: nothing was solved
  }
  EXPECT(opt.MarginalCovariance(2, &cov) && asked.back() == std::vector<int>({2}) && cov[0] == 200.0 && cov[35] == 235.0);
  EXPECT(!opt.MarginalCovariance(3, &cov) && !opt.MarginalCovariance(-1, &cov));
  EXPECT(opt.Graph().CalibNodeIndex() == 3 && opt.Graph().FrameNodeIndex() == -1);
  EXPECT(opt.CalibCovariance(&cov) && asked.back() == std::vector<int>({3}) && cov[1] == 301.0);
  EXPECT(!opt.GpsCoordCovariance(&cov));                                          // no GPS-frame vertex
  EXPECT(!opt.JointMarginalCovariance(1, 1, &joint) && !opt.JointMarginalCovariance(1, 3, &joint));
  EXPECT(opt.JointMarginalCovariance(1, 2, &joint) && asked.back() == std::vector<int>({1, 2}) && asked_rows.back() == std::vector<int>({1, 2}));
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) {
      EXPECT(joint[static_cast<size_t>(12 * a + b)] == 100.0 + 6 * a + b);                                   // Sigma_1
      EXPECT(joint[static_cast<size_t>(12 * (6 + a) + 6 + b)] == 200.0 + 6 * a + b);                         // Sigma_2
      // [H^-1]_{1,2} from query 2 (1000 x 1 + 10 x 2) averaged with the transpose of [H^-1]_{2,1} from query 1 (1000 x 2 + 10 x 1)
      const double want = 0.5 * ((1020.0 + (6 * a + b) / 100.0) + (2010.0 + (6 * b + a) / 100.0));
      EXPECT(joint[static_cast<size_t>(12 * a + 6 + b)] == want && joint[static_cast<size_t>(12 * (6 + b) + a)] == want);
    }
  // the world-frame position covariance: R Sigma_vv R^T for a quarter turn about z
  be::PoseGraph g;
  reg::Matrix4d X = reg::Matrix4d::Identity();
  X(0, 0) = 0; X(0, 1) = -1; X(1, 0) = 1; X(1, 1) = 0;
  g.AddVertex(0, X, reg::Matrix4d::Identity());
  std::array<double, 36> c{};
  c[21] = 4.0; c[28] = 9.0; c[35] = 16.0;                                        // diag(Sigma_vv) = 4, 9, 16
  const std::array<double, 9> w = g.WorldPositionCovariance(0, c);
  EXPECT(w[0] == 9.0 && w[4] == 4.0 && w[8] == 16.0 && w[1] == 0.0);
  std::printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
  return failures ? 1 : 0;
}
