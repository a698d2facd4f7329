// smhip/pose_graph.h -- back_end::IsamOptimizer (the reference's back_end/isam_optimizer.{h,cc}) restated over the device pose-graph
// optimiser (smhip_pose_graph_optimize, include/smhip.h).  Header-only, on top of smhip/back_end.h and smhip/submap.h.
//
//   IsamOptimizer::AddVertex          isam_optimizer.cc:140-173   the vertex, held constant when it is the first (the prior of sigma
//                                                                 1e-6, :78, 151, is a fixed node here), else a between-factor to
//                                                                 the previous vertex
//   IsamOptimizer::AddLoopCloseEdge   :127-138                    between(target, source) measured as transform_tgt_to_src
//   IsamOptimizer::AddFrame           :196-293                    the loop detector, the vertex, one factor per edge when
//                                                                 close_succeed, the update, UpdateAllPose (:106-125)
//   IsamOptimizer::RunFinalOptimazation :351-383, GetWholeGraph :385-387
//
// What differs from the reference, on purpose:
//   * GTSAM's iSAM2 (incremental, dogleg, :70-76) is replaced by a batch solve from the current estimate on every update; the
//     factor, its noise and the objective are DESIGN.md section 6 ("Pose graph").  Both end in the same local minimum of the same
//     objective to first order in the residual (GTSAM's Pose3 chart is not pinned by the reference's text).
//   * Not restated, and without an option here: GPS / ENU factors and SolveGpsCorrdAlone, the odometry calibration factor
//     (ODOM_CALIB_KEY), the Huber odometry model (:84-93), IMU, ViewGraph's picture output (GetWholeGraph returns the plain list),
//     the multi-trajectory optimiser.
#ifndef SMHIP_POSE_GRAPH_H_
#define SMHIP_POSE_GRAPH_H_

#include <array>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <utility>
#include <vector>

#include "smhip/back_end.h"
#include "smhip/submap.h"

namespace smhip {
namespace back_end {

using Sigmas = std::array<double, 6>;                                      // rotation first, as gtsam::Pose3
inline Sigmas FrameMatchSigmas() { return {0.1, 0.1, 0.1, 0.15, 0.15, 0.15}; }    // frame_match_noise_model_, :80-81
inline Sigmas LoopClosureSigmas() { return {0.1, 0.1, 0.1, 0.15, 0.15, 0.15}; }   // loop_closure_noise_model_, :82-83

// The vertices and between-factors, in the arrays smhip_pose_graph_optimize takes.
class PoseGraph {
 public:
  struct Edge { int i = 0, j = 0; Matrix4d transform = Matrix4d::Identity(); Sigmas sigmas = FrameMatchSigmas(); };

  // :140-173.  Vertices come in index order; vertex 0 is constant.
  void AddVertex(int index, const Matrix4d& pose, const Matrix4d& transform_from_last_pose, const Sigmas& odom_noise = FrameMatchSigmas()) {
    SMHIP_CHECK(index == static_cast<int>(poses_.size()), "vertices are added in index order");
    poses_.push_back(pose);
    fixed_.push_back(index == 0 ? 1 : 0);
    if (index > 0) AddEdge(index - 1, index, transform_from_last_pose, odom_noise);
  }
  // :127-138
  void AddLoopCloseEdge(int target_index, int source_index, const Matrix4d& transform_tgt_to_src, const Sigmas& loop_close_noise = LoopClosureSigmas()) {
    AddEdge(target_index, source_index, transform_tgt_to_src, loop_close_noise);
  }
  // One device solve from the current poses, which it replaces.  false (poses unchanged, the reason on stderr) when refused.
  bool Optimize(smhip_handle handle, smhip_pose_graph_stats* stats = nullptr, const smhip_pose_graph_options* options = nullptr) {
    SMHIP_CHECK(handle != nullptr, "PoseGraph::Optimize needs a device handle");
    if (poses_.empty()) return true;
    std::vector<double> poses, Z, sigmas;
    std::vector<int32_t> ij;
    Flatten(&poses, &ij, &Z, &sigmas);
    const smhip_status s = smhip_pose_graph_optimize(handle, static_cast<int>(poses_.size()), poses.data(), fixed_.data(), static_cast<int>(edges_.size()),
                                                     ij.data(), Z.data(), sigmas.data(), options, stats);
    if (s != SMHIP_OK) {
      std::fprintf(stderr, "[ERROR] smhip_pose_graph_optimize: %s (%s)\n", smhip_status_string(s), smhip_last_error(handle));
      return false;
    }
    SetFlatPoses(poses);
    return true;
  }
  // the C ABI's arrays: 16 doubles per pose and per measurement (column-major), index pairs, 6 sigmas per edge
  void Flatten(std::vector<double>* poses, std::vector<int32_t>* ij, std::vector<double>* Z, std::vector<double>* sigmas) const {
    poses->clear(); ij->clear(); Z->clear(); sigmas->clear();
    for (const Matrix4d& p : poses_) poses->insert(poses->end(), p.data(), p.data() + 16);
    for (const Edge& e : edges_) {
      ij->push_back(e.i); ij->push_back(e.j);
      Z->insert(Z->end(), e.transform.data(), e.transform.data() + 16);
      sigmas->insert(sigmas->end(), e.sigmas.begin(), e.sigmas.end());
    }
  }
  void SetFlatPoses(const std::vector<double>& poses) {
    SMHIP_CHECK(poses.size() == 16 * poses_.size(), "16 doubles per vertex");
    for (size_t k = 0; k < poses_.size(); ++k)
      for (int q = 0; q < 16; ++q) poses_[k].data()[q] = poses[16 * k + static_cast<size_t>(q)];
  }
  int VertexCount() const { return static_cast<int>(poses_.size()); }
  const Matrix4d& Pose(int index) const { return poses_.at(static_cast<size_t>(index)); }
  const std::vector<Matrix4d>& Poses() const { return poses_; }
  const std::vector<uint8_t>& Fixed() const { return fixed_; }
  const std::vector<Edge>& Edges() const { return edges_; }

 private:
  void AddEdge(int i, int j, const Matrix4d& transform, const Sigmas& sigmas) {
    const int n = static_cast<int>(poses_.size());
    SMHIP_CHECK(i >= 0 && j >= 0 && i < n && j < n && i != j, "an edge joins two different vertices that exist");
    Edge e;
    e.i = i; e.j = j; e.transform = transform; e.sigmas = sigmas;
    edges_.push_back(e);
  }
  std::vector<Matrix4d> poses_;
  std::vector<uint8_t> fixed_;
  std::vector<Edge> edges_;
};

struct IsamOptimizerOptions {
  int max_iterations = 50;            // of one solve (smhip_pose_graph_options)
};

// view_graph.h's GraphItem without the picture: what GetWholeGraph returns
struct GraphItem {
  int index = 0;
  Matrix4d pose = Matrix4d::Identity();
  std::vector<std::pair<int, Matrix4d>> connections;     // (the other vertex, transform to it), in the order the edges were added
};

class IsamOptimizer {
 public:
  // TEST HOOK, not part of the reference's class: `solver` replaces the device solve (tests without a device); it optimises the
  // graph in place and returns false when it could not
  using Solver = std::function<bool(PoseGraph*)>;

  IsamOptimizer(const IsamOptimizerOptions& options, const LoopDetectorSettings& l_d_setting, smhip_handle handle)
      : loop_detector_(new LoopDetector(l_d_setting)), options_(options), handle_(handle) {}
  IsamOptimizer(const IsamOptimizer&) = delete;
  IsamOptimizer& operator=(const IsamOptimizer&) = delete;
  void SetSolver(Solver solver) { solver_ = std::move(solver); }

  // :196-293.  `frame`: the submap as the detector sees it; `transform_from_last`: Submap::TransformFromLast(), the matched
  // transform from the previous submap (ignored for the first).  Every frame's global_pose is written back, which is what the
  // detector reads again on its next AddFrame.  false when a solve failed (the reason on stderr): the vertex and its factors stay in
  // the graph, every frame keeps the pose it had, and a later AddFrame or RunFinalOptimazation solves the whole graph again.
  bool AddFrame(const std::shared_ptr<LoopFrame>& frame, const Matrix4d& transform_from_last) {
    SMHIP_CHECK(frame != nullptr, "CHECK(frame)");
    const DetectResult result = loop_detector_->AddFrame(frame, true);                          // :199
    return AddDetected(frame, transform_from_last, result);
  }
  // TEST HOOK: the part of AddFrame after the detector (:200-292), for a detector result made by hand
  bool AddDetected(const std::shared_ptr<LoopFrame>& frame, const Matrix4d& transform_from_last, const DetectResult& result) {
    const int frame_index = graph_.VertexCount();
    SMHIP_CHECK(frame_index == result.current_frame_index, "CHECK_EQ(frame_index, result.current_frame_index)");   // :202
    frames_.push_back(frame);
    graph_.AddVertex(frame_index, frame->global_pose, transform_from_last, FrameMatchSigmas());  // :206-207
    bool ok = Update();                                                                         // IsamUpdate of :172
    if (result.close_succeed) {                                                                 // :227-236
      for (const LoopEdge& edge : result.edges) {
        graph_.AddLoopCloseEdge(edge.close_pair_index.first, edge.close_pair_index.second, edge.transform, LoopClosureSigmas());
        ++loop_edges_;
      }
      ok = Update() && ok;
    }
    if (ok) UpdateAllPose();                                                                    // :292
    return ok;
  }
  bool RunFinalOptimazation() {                                                                 // :351-353
    const bool ok = Update();
    if (ok) UpdateAllPose();
    return ok;
  }
  std::vector<GraphItem> GetWholeGraph() const {                                                // :385-387
    std::vector<GraphItem> out(static_cast<size_t>(graph_.VertexCount()));
    for (int k = 0; k < graph_.VertexCount(); ++k) { out[static_cast<size_t>(k)].index = k; out[static_cast<size_t>(k)].pose = graph_.Pose(k); }
    for (const PoseGraph::Edge& e : graph_.Edges()) out[static_cast<size_t>(e.i)].connections.emplace_back(e.j, e.transform);
    return out;
  }
  const PoseGraph& Graph() const { return graph_; }
  LoopDetector* GetLoopDetector() { return loop_detector_.get(); }
  int LoopEdgeCount() const { return loop_edges_; }
  int SolveCount() const { return solves_; }
  const smhip_pose_graph_stats& LastStats() const { return last_stats_; }

 private:
  // a batch solve in place of isam_->update (:96-104); a graph of one vertex has nothing to solve
  bool Update() {
    if (graph_.VertexCount() < 2) return true;
    bool ok;
    if (solver_) {
      ok = solver_(&graph_);
    } else {
      smhip_pose_graph_options o;
      smhip_pose_graph_default_options(&o);
      o.max_iterations = options_.max_iterations;
      ok = graph_.Optimize(handle_, &last_stats_, &o);
    }
    if (ok) ++solves_;
    return ok;
  }
  void UpdateAllPose() {                                                                        // :106-125
    for (size_t i = 0; i < frames_.size(); ++i) frames_[i]->global_pose = graph_.Pose(static_cast<int>(i));
  }

  std::unique_ptr<LoopDetector> loop_detector_;
  IsamOptimizerOptions options_;
  smhip_handle handle_ = nullptr;
  Solver solver_;
  PoseGraph graph_;
  std::vector<std::shared_ptr<LoopFrame>> frames_;
  smhip_pose_graph_stats last_stats_{};
  int loop_edges_ = 0, solves_ = 0;
};

}  // namespace back_end
}  // namespace smhip

#endif  // SMHIP_POSE_GRAPH_H_
