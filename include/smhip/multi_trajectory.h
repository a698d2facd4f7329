// smhip/multi_trajectory.h -- joining a second drive to a finished map: back_end::MultiTrajectoryOptimizer (the reference's
// back_end/multi_trajectory/multi_trajectory_optimizer.{h,cc}) and MultiTrajectoryMapBuilder
// (builder/multi_trajectory/multi_trajectory_map_builder.{h,cc}) restated over the device pose graph (smhip/pose_graph.h), the loop
// detector (smhip/back_end.h) and the map files (smhip/trajectory_map.h).  Header-only.  No kernel is added: the device work of a join
// is smhip_m2dp_f32 (a loaded submap's descriptor), IcpPointMatcherHip (the cross-trajectory matches), one pose-graph solve,
// smhip_submap_build_f32 (the whole-map PCD) and smhip_mrvm_insert_transformed_f32 (the static map).
//
//   MultiTrajectoryOptimizer::AddSubmap              :88-112    the detector, the vertex (a prior on a trajectory's first submap,
//                                                                :150-166), one loop factor per edge when close_succeed
//   MultiTrajectoryOptimizer::AddSubmapConnection    :114-147   between(target, source); a loop constraint is also noted in the target's
//                                                                connection list
//   MultiTrajectoryOptimizer::UseCurrentStateAsBaseMap :169-177 SetSearchWindow(0, frames - 1): SelectLoopCandidates loops i < end, so the
//                                                                LAST base submap is never a candidate -- kept as the reference has it
//   MultiTrajectoryOptimizer::RunFinalOptimizing     :180-194   every submap's pose written back
//   MultiTrajectoryMapBuilder::LoadBaseMap           :50-83     LoadIncrementalMap :85-138, SaveWholeMap :214-228,
//                                                                GenerateWholeMapPcd :230-247, GenerateStaticMap :249-275
//
// The graph.  A submap's node is its place in the concatenation: trajectories in order, submaps in index order, so consecutive
// submaps of one trajectory are consecutive nodes -- the chain the preconditioner solves exactly.  Factors: a PRIOR of sigma 0.1 x 6 at
// the loaded pose on the first submap of every trajectory (:66-67, 156-160); connections sigma 0.01 x 6 (stable_odom_model_); loop
// constraints sigma 0.025 x 6 under Huber(loop_closure_huber = 1) (loop_closure_model_).
//
// What differs from the reference, on purpose ("Joining maps"):
//   * One solve.  The reference's isam_->update() after every vertex and factor only keeps iSAM current: submap poses change in
//     RunFinalOptimizing and nowhere else, so the detector sees loaded poses throughout.  Here nothing is solved before
//     RunFinalOptimizing, which runs one batch solve of the device pose graph.
//   * connection_huber.  The reference also puts Huber(1) on its connection factors (stable_odom_model_, :68-71).  Thresholds on chain
//     edges converge slowly (include/smhip.h, "Robust factors"): on a joined graph of 8 + 8 submaps with the base held it costs 23 steps
//     instead of 19 and moves the submaps that carry loop edges by less than 1 cm.  The option's default is 0 (none); 1.0 is the reference.
//   * hold_base_map (default false, the reference): every node present at UseCurrentStateAsBaseMap is held (PoseGraph::HoldVertex)
//     and the priors of the trajectories begun before it are left out -- so with this option set, nothing can be solved before
//     UseCurrentStateAsBaseMap.  Every cross edge then lands in a diagonal block, which the preconditioner holds exactly, and the base
//     poses keep their bits: the mode for large maps and for a base that has been published.
//   * The reference CHECKs; here a same-trajectory loop edge, an id out of order and a graph beyond SMHIP_POSE_GRAPH_MAX_NODES /
//     SMHIP_POSE_GRAPH_MAX_EDGES are refused: false, the reason in LastError(), the graph as it was.
//   * GenerateWholeMapPcd writes DATA binary through smhip/pcd.h where the reference writes binary_compressed.
//   * ViewGraph's picture (multi_graph.jpg) is not restated.
#ifndef SMHIP_MULTI_TRAJECTORY_H_
#define SMHIP_MULTI_TRAJECTORY_H_

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <list>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "smhip/mrvm.h"
#include "smhip/pcd.h"
#include "smhip/pose_graph.h"
#include "smhip/trajectory_map.h"

namespace smhip {
namespace back_end {

using builder::SubmapId;

inline Sigmas MultiTrajectoryPriorSigmas() { return {0.1, 0.1, 0.1, 0.1, 0.1, 0.1}; }                  // prior_noise_model_, :66-67
inline Sigmas MultiTrajectoryConnectionSigmas() { return {0.01, 0.01, 0.01, 0.01, 0.01, 0.01}; }       // stable_odom_model_, :68-71
inline Sigmas MultiTrajectoryLoopSigmas() { return {0.025, 0.025, 0.025, 0.025, 0.025, 0.025}; }       // loop_closure_model_, :77-81

// What a connection is measured as: target^-1 * source of the loaded poses, in double, evaluated the way the device evaluates
// X_i^-1 X_j in a between-factor's residual (csrc/pose_graph_kernel.h, edge_error): R = R_t^T R_s and t = R_t^T (t_s - t_t), every
// three-term sum x0 y0 + x1 y1 + x2 y2 contracted as the gfx950 code object has it, fma(x2, y2, fma(x0, y0, x1 y1)).  The factor's
// residual at the loaded poses is then exactly zero on the device -- Z^T (R_t^T R_s) is a product of a matrix with its own bits and
// comes out exactly symmetric, and the translations are the same bits -- so a map that is loaded and solved alone starts at cost 0
// and keeps every bit.  In any other arithmetic (the kernel's loop compiled for the CPU without contraction) the residual is a few
// ulp instead.
inline Matrix4d ConnectionTransform(const Matrix4d& target, const Matrix4d& source) {
  Matrix4d z = Matrix4d::Identity();
  const double d[3] = {source(0, 3) - target(0, 3), source(1, 3) - target(1, 3), source(2, 3) - target(2, 3)};
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) z(a, b) = std::fma(target(2, a), source(2, b), std::fma(target(0, a), source(0, b), target(1, a) * source(1, b)));
    z(a, 3) = std::fma(target(2, a), d[2], std::fma(target(0, a), d[0], target(1, a) * d[1]));
  }
  return z;
}

struct MultiTrajectoryOptions {
  int max_iterations = 50;            // of the one solve (smhip_pose_graph_options)
  double loop_closure_huber = 1.0;    // the Huber threshold of every loop constraint (:77-81); 0: none
  double connection_huber = 0.0;      // ... of every other connection; 0: none (a deviation, see above), 1.0: the reference (:68-71)
  bool hold_base_map = false;         // hold every node present at UseCurrentStateAsBaseMap and leave the base priors out
};

class MultiTrajectoryOptimizer {
 public:
  // TEST HOOKS, as IsamOptimizer's: `solver` replaces the device solve, `reporter` PoseGraph::Report
  using Solver = std::function<bool(PoseGraph*)>;
  using Reporter = std::function<bool(const PoseGraph&, std::vector<double>* norm, std::vector<double>* weight)>;

  MultiTrajectoryOptimizer(const MultiTrajectoryOptions& options, const LoopDetectorSettings& l_d_setting, smhip_handle handle)
      : loop_detector_(new LoopDetector(l_d_setting)), options_(options), handle_(handle) {
    SMHIP_CHECK(std::isfinite(options.loop_closure_huber) && options.loop_closure_huber >= 0.0, "loop_closure_huber is finite and not negative");
    SMHIP_CHECK(std::isfinite(options.connection_huber) && options.connection_huber >= 0.0, "connection_huber is finite and not negative");
  }
  MultiTrajectoryOptimizer(const MultiTrajectoryOptimizer&) = delete;
  MultiTrajectoryOptimizer& operator=(const MultiTrajectoryOptimizer&) = delete;
  void SetSolver(Solver solver) { solver_ = std::move(solver); }
  void SetReporter(Reporter reporter) { reporter_ = std::move(reporter); }

  // :88-112.  Submaps come trajectory by trajectory and, within one, in index order from 0.
  bool AddSubmap(const std::shared_ptr<LoopFrame>& frame, const SubmapId& id, bool do_loop_detect) {
    SMHIP_CHECK(frame != nullptr, "CHECK(submap)");
    if (!IdIsNext(id) || !RoomFor(1, FirstOfTrajectoryGetsPrior(id) ? 1 : 0)) return false;
    const DetectResult result = loop_detector_->AddFrame(frame, do_loop_detect);                // :95-96
    return AddDetectedChecked(frame, id, result);
  }
  // TEST HOOK: the part of AddSubmap after the detector, for a detector result made by hand (the frame enters the detector without a search)
  bool AddDetected(const std::shared_ptr<LoopFrame>& frame, const SubmapId& id, const DetectResult& result) {
    SMHIP_CHECK(frame != nullptr, "CHECK(submap)");
    if (!IdIsNext(id) || !RoomFor(1, FirstOfTrajectoryGetsPrior(id) ? 1 : 0)) return false;
    loop_detector_->AddFrame(frame, false);
    return AddDetectedChecked(frame, id, result);
  }
  // :114-147.  transform: the source's pose in the target's frame.
  bool AddSubmapConnection(const SubmapId& target, const SubmapId& source, const Matrix4d& transform, bool is_loop_constraint) {
    const int t = NodeOf(target), s = NodeOf(source);
    if (t < 0 || s < 0) return Refuse("a connection between " + target.DebugString() + " and " + source.DebugString() + " names a submap that was not added");
    if (t == s) return Refuse("a connection joins " + target.DebugString() + " to itself");
    if (is_loop_constraint && target.trajectory_index == source.trajectory_index)                // CHECK_NE, :105
      return Refuse("a loop constraint between " + target.DebugString() + " and " + source.DebugString() + " joins two submaps of one trajectory");
    if (!RoomFor(0, 1)) return false;
    if (is_loop_constraint) {
      connections_[static_cast<size_t>(t)].push_back(source);                                   // :120-125
      loop_edge_at_.push_back(static_cast<int>(graph_.Edges().size()));
      graph_.AddLoopCloseEdge(t, s, transform, MultiTrajectoryLoopSigmas(), options_.loop_closure_huber);
    } else {
      graph_.AddLoopCloseEdge(t, s, transform, MultiTrajectoryConnectionSigmas(), options_.connection_huber);
    }
    solved_ = false;
    return true;
  }
  // :169-177
  void UseCurrentStateAsBaseMap() {
    const int frames = static_cast<int>(loop_detector_->GetFrames().size());
    if (frames == 0) return;
    loop_detector_->SetSearchWindow(0, frames - 1);
    base_nodes_ = frames;
    base_marked_ = true;
    if (options_.hold_base_map)
      for (int k = 0; k < frames; ++k) graph_.HoldVertex(k);
  }
  // :180-194: the one solve, then every submap's pose written back.  false (every pose as it was, the reason in LastError() or on
  // stderr) when the solve was refused or failed.
  bool RunFinalOptimizing() {
    bool any_free = false;
    for (uint8_t f : graph_.Fixed()) any_free = any_free || f == 0;
    if (graph_.VertexCount() == 0 || !any_free) return true;                                    // nothing to solve: every node is held
    bool ok;
    if (solver_) {
      ok = solver_(&graph_);
    } else {
      smhip_pose_graph_options o;
      smhip_pose_graph_default_options(&o);
      o.max_iterations = options_.max_iterations;
      ok = graph_.Optimize(handle_, &last_stats_, &o);
    }
    solved_ = ok;
    if (!ok) return Refuse("the pose graph could not be optimised");
    ++solves_;
    for (size_t i = 0; i < frames_.size(); ++i) frames_[i]->global_pose = graph_.Pose(static_cast<int>(i));
    return true;
  }

  const PoseGraph& Graph() const { return graph_; }
  LoopDetector* GetLoopDetector() { return loop_detector_.get(); }
  int TrajectoryCount() const { return static_cast<int>(start_.size()); }
  int SubmapCount(int trajectory) const { return count_.at(static_cast<size_t>(trajectory)); }
  int BaseNodeCount() const { return base_nodes_; }
  // the node of a submap, or -1
  int NodeOf(const SubmapId& id) const {
    if (id.trajectory_index < 0 || id.trajectory_index >= TrajectoryCount()) return -1;
    if (id.submap_index < 0 || id.submap_index >= count_[static_cast<size_t>(id.trajectory_index)]) return -1;
    return start_[static_cast<size_t>(id.trajectory_index)] + id.submap_index;
  }
  const SubmapId& IdOf(int node) const { return ids_.at(static_cast<size_t>(node)); }
  // the loop constraints' sources noted for a target, in the order added (Submap::AddConnectedSubmap, :120-125)
  const std::vector<SubmapId>& LoopConnections(const SubmapId& target) const { return connections_.at(static_cast<size_t>(NodeOf(target))); }
  int LoopEdgeCount() const { return static_cast<int>(loop_edge_at_.size()); }
  int SolveCount() const { return solves_; }
  const smhip_pose_graph_stats& LastStats() const { return last_stats_; }
  const std::string& LastError() const { return error_; }
  // Every loop constraint, in the order added, with its norm and weight at the poses of the solve (nodes as target and source).
  // Empty when there is none, nothing was solved since the last change or the report was refused.
  std::vector<LoopEdgeWeight> LoopEdgeReport() const {
    std::vector<LoopEdgeWeight> out;
    if (loop_edge_at_.empty() || !solved_) return out;
    std::vector<double> norm, weight;
    if (!(reporter_ ? reporter_(graph_, &norm, &weight) : graph_.Report(handle_, &norm, &weight, nullptr))) return out;
    for (int at : loop_edge_at_) {
      const PoseGraph::Edge& e = graph_.Edges()[static_cast<size_t>(at)];
      LoopEdgeWeight w;
      w.target = e.i; w.source = e.j; w.norm = norm[static_cast<size_t>(at)]; w.weight = weight[static_cast<size_t>(at)];
      out.push_back(w);
    }
    return out;
  }

 private:
  bool Refuse(const std::string& why) { error_ = why; return false; }
  bool IdIsNext(const SubmapId& id) {
    const int T = TrajectoryCount();
    const bool continues = T > 0 && id.trajectory_index == T - 1 && id.submap_index == count_.back();
    const bool begins = id.trajectory_index == T && id.submap_index == 0;
    if (continues || begins) return true;
    return Refuse("submap " + id.DebugString() + " is out of order: submaps come trajectory by trajectory and in index order from 0 (" + std::to_string(T) +
                  " trajectories so far" + (T > 0 ? ", the last with " + std::to_string(count_.back()) + " submaps)" : ")"));
  }
  bool FirstOfTrajectoryGetsPrior(const SubmapId& id) const { return id.submap_index == 0 && !(options_.hold_base_map && !base_marked_); }
  bool RoomFor(int more_nodes, int more_factors) {
    const int nodes = graph_.NodeCount() + more_nodes, factors = graph_.FactorCount() + more_factors;
    if (nodes <= SMHIP_POSE_GRAPH_MAX_NODES && factors <= SMHIP_POSE_GRAPH_MAX_EDGES) return true;
    return Refuse("the joined graph would have " + std::to_string(nodes) + " nodes and " + std::to_string(factors) + " factors; one device solve takes at most " +
                  std::to_string(SMHIP_POSE_GRAPH_MAX_NODES) + " nodes and " + std::to_string(SMHIP_POSE_GRAPH_MAX_EDGES) + " factors");
  }
  bool AddDetectedChecked(const std::shared_ptr<LoopFrame>& frame, const SubmapId& id, const DetectResult& result) {
    if (result.close_succeed) {                                                                 // checked before anything enters the graph
      for (const LoopEdge& edge : result.edges) {
        const int t = edge.close_pair_index.first, s = edge.close_pair_index.second;
        const int n = graph_.VertexCount();
        if (t < 0 || t >= n || s != n) return Refuse("a detected edge does not join an earlier submap to " + id.DebugString());
        if (ids_[static_cast<size_t>(t)].trajectory_index == id.trajectory_index)              // CHECK_NE, :105
          return Refuse("a loop constraint between " + ids_[static_cast<size_t>(t)].DebugString() + " and " + id.DebugString() + " joins two submaps of one trajectory");
      }
      if (!RoomFor(1, static_cast<int>(result.edges.size()) + (FirstOfTrajectoryGetsPrior(id) ? 1 : 0))) return false;
    }
    if (id.submap_index == 0) { start_.push_back(graph_.VertexCount()); count_.push_back(0); }
    ++count_.back();
    frames_.push_back(frame);
    ids_.push_back(id);
    connections_.emplace_back();
    const int node = graph_.AddLooseVertex(frame->global_pose);                                 // AddVertex, :150-166
    if (FirstOfTrajectoryGetsPrior(id)) graph_.AddPriorFactor(node, frame->global_pose, MultiTrajectoryPriorSigmas());
    solved_ = false;
    if (result.close_succeed)                                                                   // :99-111
      for (const LoopEdge& edge : result.edges)
        if (!AddSubmapConnection(ids_[static_cast<size_t>(edge.close_pair_index.first)], id, edge.transform, true)) return false;
    return true;
  }

  std::unique_ptr<LoopDetector> loop_detector_;
  MultiTrajectoryOptions options_;
  smhip_handle handle_ = nullptr;
  Solver solver_;
  Reporter reporter_;
  PoseGraph graph_;
  std::vector<std::shared_ptr<LoopFrame>> frames_;          // by node
  std::vector<SubmapId> ids_;                               // by node
  std::vector<std::vector<SubmapId>> connections_;          // by node: the loop constraints' sources
  std::vector<int> start_, count_;                          // by trajectory: its first node, its submaps
  std::vector<int> loop_edge_at_;                           // the loop constraints' places in graph_.Edges()
  int base_nodes_ = 0, solves_ = 0;
  bool base_marked_ = false, solved_ = false;
  smhip_pose_graph_stats last_stats_{};
  std::string error_;
};

}  // namespace back_end

// ---- MultiTrajectoryMapBuilder ----------------------------------------------------------------------------------------------------

struct MultiTrajectoryMapBuilderOptions {
  back_end::LoopDetectorSettings loop_detect_settings;
  back_end::MultiTrajectoryOptions optimizer;
  int max_clouds_in_memory = 64;       // submap clouds kept after a CloseLoop asked for them; the oldest use goes first
  int device = 0;                      // of the static map (the handle's own device serves everything else)
  int static_map_table_log2 = 22;      // GenerateStaticMap's first voxel-table size
};

// Every call returns false with the reason in LastError() when it could not do its work; nothing aborts on a bad file.  `handle`: the
// device handle the descriptors, the solve and the whole-map PCD run on (its max_source_points / max_target_points bound one
// submap's cloud for the descriptor and one launch of the PCD's transform); null is allowed with the optimizer's Solver hook and
// use_descriptor = false, for tests without a device.
class MultiTrajectoryMapBuilder {
 public:
  MultiTrajectoryMapBuilder(const MultiTrajectoryMapBuilderOptions& options, smhip_handle handle, int handle_max_points = 1 << 18)
      : options_(options), handle_(handle), handle_max_points_(handle_max_points), optimizer_(options.optimizer, options.loop_detect_settings, handle) {}
  MultiTrajectoryMapBuilder(const MultiTrajectoryMapBuilder&) = delete;
  MultiTrajectoryMapBuilder& operator=(const MultiTrajectoryMapBuilder&) = delete;

  back_end::MultiTrajectoryOptimizer* Optimizer() { return &optimizer_; }
  const builder::TrajectoryMap& Map() const { return map_; }
  const std::string& LastError() const { return error_; }
  int CloudsInMemory() const { return static_cast<int>(cache_.size()); }
  long long CloudLoads() const { return cloud_loads_; }
  int BaseSubmapCount() const { return base_submaps_; }
  int IncrementalSubmapCount() const { return incremental_submaps_; }
  double SolveSeconds() const { return solve_seconds_; }               // of the last LoadIncrementalMap's one solve, as the host sees it

  // :50-83
  bool LoadBaseMap(const std::string& package_file) {
    if (!map_.trajectories.empty()) return Refuse("LoadBaseMap: a base map is already loaded");
    builder::TrajectoryMap loaded;
    if (!builder::ReadTrajectoryMap(package_file, &loaded, &error_)) return false;
    if (!AddToOptimizer(loaded, false)) return false;
    map_ = std::move(loaded);
    base_submaps_ = static_cast<int>(map_.SubmapCount());
    optimizer_.UseCurrentStateAsBaseMap();
    return true;
  }
  // :85-138: the file's trajectories and connections offset by the number of trajectories already there (:94-105, 121), submaps added
  // with loop detection against the base, the one solve, then the trajectories join the base (:134-137) -- a further map can follow.
  bool LoadIncrementalMap(const std::string& package_file) {
    if (map_.trajectories.empty()) return Refuse("LoadIncrementalMap: no base map is loaded");
    builder::TrajectoryMap loaded;
    const double base[2] = {map_.base_x, map_.base_y};
    if (!builder::ReadTrajectoryMap(package_file, &loaded, &error_, base)) return false;
    const int offset = static_cast<int>(map_.trajectories.size());
    for (builder::MapTrajectory& t : loaded.trajectories) {
      t.id += offset;
      for (builder::MapSubmap& s : t.submaps) {
        s.id.trajectory_index += offset;
        for (builder::SubmapId& c : s.connections) c.trajectory_index += offset;
      }
    }
    optimizer_.UseCurrentStateAsBaseMap();                      // (after an earlier incremental map: everything so far is the base)
    if (!AddToOptimizer(loaded, true)) return false;
    const auto t0 = std::chrono::steady_clock::now();
    if (!optimizer_.RunFinalOptimizing()) return Refuse("LoadIncrementalMap: " + optimizer_.LastError());
    solve_seconds_ = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    incremental_submaps_ = static_cast<int>(loaded.SubmapCount());
    for (builder::MapTrajectory& t : loaded.trajectories) map_.trajectories.push_back(std::move(t));
    // poses and connections back into the map: a held node keeps the numbers it was read with
    size_t node = 0;
    for (builder::MapTrajectory& t : map_.trajectories)
      for (builder::MapSubmap& s : t.submaps) {
        const bool held = optimizer_.Graph().Fixed()[node] != 0;
        if (!held) s.SetPose(frames_[node]->global_pose);
        const std::vector<builder::SubmapId>& loops = optimizer_.LoopConnections(s.id);
        for (size_t k = noted_[node]; k < loops.size(); ++k) s.connections.push_back(loops[k]);
        noted_[node] = loops.size();
        ++node;
      }
    return true;
  }
  // :214-228
  bool SaveWholeMap(const std::string& package_file) {
    if (map_.trajectories.empty()) return Refuse("SaveWholeMap: no map is loaded");
    // the submap files stay where they are: a file beside the new xml keeps its name, any other is written as its absolute path
    builder::TrajectoryMap out = map_;
    const std::string dir = builder::FilePath(package_file);
    for (builder::MapTrajectory& t : out.trajectories)
      for (builder::MapSubmap& s : t.submaps) {
        if (s.dir == dir || (!s.file.empty() && s.file[0] == '/')) continue;
        char* full = ::realpath(s.Path().c_str(), nullptr);
        if (!full) return Refuse("SaveWholeMap: submap file does not exist: " + s.Path());
        s.file = full;
        std::free(full);
      }
    return builder::WriteTrajectoryMap(package_file, out, &error_);
  }
  // :230-247: every submap's cloud moved by its pose and concatenated -- on the device (smhip_submap_build_f32 with voxel size 0,
  // as many submaps per launch as the handle takes).  DATA binary where the reference writes binary_compressed.
  bool GenerateWholeMapPcd(const std::string& pcd_filename) {
    if (!handle_) return Refuse("GenerateWholeMapPcd needs a device handle");
    std::vector<float> rows;                                                // x y z intensity
    std::vector<std::shared_ptr<data::InnerCloudType>> chunk;
    std::vector<double> chunk_poses;
    long long chunk_points = 0;
    auto flush = [&]() {
      if (chunk.empty()) return true;
      std::vector<const float*> ptr;
      std::vector<int> n;
      for (const auto& c : chunk) { ptr.push_back(c->points.empty() ? nullptr : &c->points[0].x); n.push_back(static_cast<int>(c->points.size())); }
      int m = 0;
      smhip_status st = smhip_submap_build_f32(handle_, static_cast<int>(chunk.size()), ptr.data(), 5, n.data(), chunk_poses.data(), 0.f, &m);
      std::vector<data::InnerPointType> moved(static_cast<size_t>(m > 0 ? m : 0));
      if (st == SMHIP_OK && m > 0) st = smhip_filter_get_output(handle_, &moved[0].x, nullptr, m);
      if (st != SMHIP_OK) return Refuse(std::string("GenerateWholeMapPcd: ") + smhip_status_string(st) + " (" + smhip_last_error(handle_) + ")");
      for (const data::InnerPointType& p : moved) { rows.push_back(p.x); rows.push_back(p.y); rows.push_back(p.z); rows.push_back(p.intensity); }
      chunk.clear(); chunk_poses.clear(); chunk_points = 0;
      return true;
    };
    for (const builder::MapTrajectory& t : map_.trajectories)
      for (const builder::MapSubmap& s : t.submaps) {
        std::shared_ptr<data::InnerCloudType> cloud(new data::InnerCloudType);
        if (!builder::ReadSubmapCloud(s.Path(), cloud.get(), &error_)) return false;
        if (cloud->points.empty()) continue;
        if (static_cast<long long>(cloud->points.size()) > handle_max_points_)
          return Refuse("GenerateWholeMapPcd: submap " + s.id.DebugString() + " has " + std::to_string(cloud->points.size()) + " points, the handle takes " + std::to_string(handle_max_points_));
        if (chunk_points + static_cast<long long>(cloud->points.size()) > handle_max_points_ && !flush()) return false;
        chunk_points += static_cast<long long>(cloud->points.size());
        chunk_poses.insert(chunk_poses.end(), s.pose.data(), s.pose.data() + 16);
        chunk.push_back(cloud);
      }
    if (!flush()) return false;
    if (rows.empty()) return Refuse("GenerateWholeMapPcd: the map has no points");
    if (!pcd::SaveBinary(pcd_filename, rows.data(), rows.size() / 4, false)) return Refuse("GenerateWholeMapPcd: cannot write " + pcd_filename);
    whole_map_points_ = static_cast<long long>(rows.size() / 4);
    return true;
  }
  // :249-275: the reference's settings -- z_offset 1.2, max_point_num_in_cell 4, output threshold 0.57 -- and every submap's cloud
  // inserted under its pose with origin = the pose's translation (smhip_mrvm_insert_transformed_f32)
  bool GenerateStaticMap(const std::string& pcd_filename) {
    MrvmSettings settings;
    settings.z_offset = 1.2f;
    settings.max_point_num_in_cell = 4;
    size_t largest = 1;
    std::vector<std::shared_ptr<data::InnerCloudType>> clouds;              // (one at a time below; sized first)
    for (const builder::MapTrajectory& t : map_.trajectories)
      for (const builder::MapSubmap& s : t.submaps) {
        data::InnerCloudType c;
        if (!builder::ReadSubmapCloud(s.Path(), &c, &error_)) return false;
        largest = std::max(largest, c.points.size());
      }
    MultiResolutionVoxelMapHip map(options_.device, options_.static_map_table_log2, static_cast<int>(largest));
    map.Initialise(settings);
    for (const builder::MapTrajectory& t : map_.trajectories)
      for (const builder::MapSubmap& s : t.submaps) {
        data::InnerCloudType c;
        if (!builder::ReadSubmapCloud(s.Path(), &c, &error_)) return false;
        if (c.points.empty()) continue;
        if (!map.InsertPointCloud(c.points, s.pose)) return Refuse("GenerateStaticMap: the device refused submap " + s.id.DebugString());
      }
    static_map_voxels_ = map.VoxelCount();
    if (!map.OutputToPointCloud(0.57f, pcd_filename, false)) return Refuse("GenerateStaticMap: nothing written to " + pcd_filename);
    return true;
  }
  long long WholeMapPoints() const { return whole_map_points_; }
  int StaticMapVoxels() const { return static_map_voxels_; }

 private:
  bool Refuse(const std::string& why) { error_ = why; return false; }
  // a submap's cloud as CloseLoop matches it (Submap::Cloud(): read from disk, normals calculated, submap.cc:160-161), through the
  // bounded cache
  back_end::InnerCloudPtr LoadCloud(const std::string& path) {
    for (auto it = cache_.begin(); it != cache_.end(); ++it)
      if (it->first == path) { cache_.splice(cache_.begin(), cache_, it); return cache_.front().second; }
    data::InnerCloudType raw;
    std::string why;
    if (!builder::ReadSubmapCloud(path, &raw, &why)) { std::fprintf(stderr, "[ERROR] %s\n", why.c_str()); return back_end::InnerCloudPtr(); }
    back_end::InnerCloudPtr cloud(new data::InnerPointCloudData(raw.points));
    if (!raw.points.empty()) cloud->CalculateNormals();
    ++cloud_loads_;
    cache_.emplace_front(path, cloud);
    while (static_cast<int>(cache_.size()) > std::max(2, options_.max_clouds_in_memory)) cache_.pop_back();   // (a match needs two)
    return cloud;
  }
  // step 2 and step 3 of :56-80 / :97-128 for the trajectories of `loaded` (ids already offset): the submaps, then their connections
  // measured as target^-1 * source of the loaded poses (ConnectionTransform) -- so every connection's residual is zero as loaded
  bool AddToOptimizer(const builder::TrajectoryMap& loaded, bool do_loop_detect) {
    smhip_m2dp_options mo;
    int dlen = 0;
    if (options_.loop_detect_settings.use_descriptor) {
      if (!handle_) return Refuse("use_descriptor needs a device handle");
      smhip_m2dp_default_options(&mo);
      dlen = smhip_m2dp_length(&mo);
    }
    std::map<builder::SubmapId, back_end::Matrix4d> pose_of;
    for (const builder::MapTrajectory& t : map_.trajectories) for (const builder::MapSubmap& s : t.submaps) pose_of[s.id] = s.pose;
    for (const builder::MapTrajectory& t : loaded.trajectories) for (const builder::MapSubmap& s : t.submaps) pose_of[s.id] = s.pose;
    for (const builder::MapTrajectory& t : loaded.trajectories)
      for (const builder::MapSubmap& s : t.submaps) {
        std::shared_ptr<back_end::LoopFrame> frame(new back_end::LoopFrame);
        frame->global_pose = s.pose;
        const std::string path = s.Path();
        frame->cloud_loader = [this, path]() { return LoadCloud(path); };
        if (dlen > 0) {                                                     // the descriptor of a loaded submap, on the device
          data::InnerCloudType raw;
          if (!builder::ReadSubmapCloud(path, &raw, &error_)) return false;
          frame->descriptor.resize(static_cast<size_t>(dlen));
          const smhip_status st = smhip_m2dp_f32(handle_, raw.points.empty() ? nullptr : &raw.points[0].x, 5, static_cast<int>(raw.points.size()), &mo, frame->descriptor.data(), dlen);
          if (st != SMHIP_OK) return Refuse("descriptor of submap " + s.id.DebugString() + ": " + smhip_status_string(st) + " (" + smhip_last_error(handle_) + ")");
        }
        if (!optimizer_.AddSubmap(frame, s.id, do_loop_detect)) return Refuse(optimizer_.LastError());
        frames_.push_back(frame);
        noted_.push_back(0);
      }
    for (const builder::MapTrajectory& t : loaded.trajectories)
      for (const builder::MapSubmap& s : t.submaps)
        for (const builder::SubmapId& c : s.connections) {
          const auto source = pose_of.find(c);
          if (source == pose_of.end()) return Refuse("connection of " + s.id.DebugString() + " names " + c.DebugString() + ", which does not exist");
          if (!optimizer_.AddSubmapConnection(s.id, c, back_end::ConnectionTransform(s.pose, source->second), false)) return Refuse(optimizer_.LastError());
        }
    return true;
  }

  MultiTrajectoryMapBuilderOptions options_;
  smhip_handle handle_ = nullptr;
  long long handle_max_points_ = 0;
  back_end::MultiTrajectoryOptimizer optimizer_;
  builder::TrajectoryMap map_;                                              // base trajectories (the incremental ones after their solve)
  std::vector<std::shared_ptr<back_end::LoopFrame>> frames_;                // by node
  std::vector<size_t> noted_;                                               // by node: loop connections already copied into map_
  std::list<std::pair<std::string, back_end::InnerCloudPtr>> cache_;        // most recently used first
  long long cloud_loads_ = 0, whole_map_points_ = 0;
  double solve_seconds_ = 0.0;
  int base_submaps_ = 0, incremental_submaps_ = 0, static_map_voxels_ = 0;
  std::string error_;
};

}  // namespace smhip

#endif  // SMHIP_MULTI_TRAJECTORY_H_
