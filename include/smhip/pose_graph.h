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
//   the GPS / ENU factors           :238-293                      use_gps: a frame's ENU fix is cached until gps_factor_init_num are there
//                                                                 and the drive has turned by gps_factor_init_angle_rad
//                                                                 (AnalyseAllFramePoseForMaxRotation, :175-194); the frame that
//                                                                 finds both runs SolveGpsCorrdAlone, gives every cached frame its
//                                                                 factor and is itself neither cached nor given one (:271-279);
//                                                                 afterwards every gps_factor_sample_step-th frame gets a factor
//   IsamOptimizer::SolveGpsCorrdAlone :295-349                    the main graph solved, then a graph of its own through the same
//                                                                 device call: the cached poses with a prior of sigma 1e-2, the frame
//                                                                 vertex (GPS_COORD_KEY: the map origin in the GPS frame) with a
//                                                                 prior of (0.2, 0.2, 1.57, 20, 20, 20) at gps_coord_transform_, one
//                                                                 factor per cached fix; its result enters the main graph with a
//                                                                 prior of (0.1, 0.1, 0.2, 1, 1, 1).  The reference stops that
//                                                                 Gauss-Newton at a relative error of 1e-6 (:330); here the stop
//                                                                 rules of smhip_pose_graph_optimize apply, with max_iterations 100
//   IsamOptimizer::GetGpsCoordTransform :370-383
//   marginal covariances             isam_optimizer.h:32          what gtsam/nonlinear/Marginals.h is included for: PoseGraph::Marginals,
//                                                                 IsamOptimizer::MarginalCovariance / JointMarginalCovariance / CalibCovariance /
//                                                                 GpsCoordCovariance over smhip_pose_graph_marginals (include/smhip.h, "Marginal
//                                                                 covariances": the chart, the gauge and what is out of scope)
//   the odometry calibration factor  :84-93, 153-162, 209-224,    use_odom: vertex 0 brings the calibration vertex (ODOM_CALIB_KEY) at tf_odom_lidar^-1,
//                                    361-367                      and every frame with an odometer reading a HANDEYE factor (include/smhip.h,
//                                                                 "Odometry calibration factor") of sigmas (0.2, 0.2, 0.2, 1.5, 1.5, 2) under
//                                                                 Huber(odom_huber = 1); RunFinalOptimazation writes tf_odom_lidar back
//
// What differs from the reference, on purpose:
//   * GTSAM's iSAM2 (incremental, dogleg, :70-76) is replaced by a batch solve from the current estimate on every update; the
//     factor, its noise and the objective are DESIGN.md section 6 ("Pose graph").  Both end in the same local minimum of the same
//     objective to first order in the residual (GTSAM's Pose3 chart is not pinned by the reference's text).
//   * The ENU factor is transformFrom(compose(GPS_COORD, pose), tracking_gps_translation) measured as enu (:238-261) to first order
//     in the residual: the POINT factor of include/smhip.h.  AnalyseAllFramePoseForMaxRotation clamps the dot product to [-1, 1]
//     before acos (the reference's can be NaN for two equal rotations, which compares as "not below the angle").  A
//     SolveGpsCorrdAlone that fails leaves nothing behind: the next frame with a fix tries again.
//   * The reference's IsamOptimizer puts its Robust(Huber(1), ...) on the odometry calibration factor alone (:84-93):
//     IsamOptimizerOptions::odom_huber; its loop edges are plain.  The multi-trajectory optimiser puts Huber(1) on every between-factor, its
//     loop_closure_model_ among them (multi_trajectory_optimizer.cc:68-81).  IsamOptimizerOptions::loop_closure_huber offers that
//     model for the loop edges here: 0 (the default) is the reference's IsamOptimizer, 1.0 the multi-trajectory optimiser's loop
//     model.  The chain edges have no option: thresholds there make the loop converge slowly (include/smhip.h, "Robust factors").
//   * Whether the calibration is estimated is an option of its own, odom_extrinsic_calib, in place of enable_extrinsic_calib (which
//     also creates the GPS tf_error point and stays refused).  Held (the default), the calibration vertex is a fixed node where the
//     reference has a prior of sigma 1e-6 (:87-88), for the reason DESIGN.md section 6 gives for node 0; free, it carries the
//     reference's prior of (0.5, 0.5, 1.5, 0.1, 0.1, 0.1) (:85-86).  The vertex starts at tf_odom_lidar^-1 itself: the reference's
//     detour through Euler angles (:154-157) is the same matrix up to rounding.
//   * Not restated, and without an option here: IMU, ViewGraph's picture output (GetWholeGraph returns the plain list), the
//     geodetic conversion to ENU, the loop detector's commented-out GPS guess (loop_detector.cc:291-300).  The tf_error
//     calibration point (GPS_CALIB_KEY) is not created: enable_extrinsic_calib = true is refused.
#ifndef SMHIP_POSE_GRAPH_H_
#define SMHIP_POSE_GRAPH_H_

#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "smhip/back_end.h"
#include "smhip/edge_information.h"
#include "smhip/submap.h"

namespace smhip {
namespace back_end {

// (Sigmas, FrameMatchSigmas() and LoopClosureSigmas() -- :80-83 -- live in smhip/edge_information.h, which floors on them)
inline std::array<double, 3> GpsSigmas() { return {0.15, 0.15, 0.15}; }            // gps_noise_model_, :79
inline Sigmas GpsCoordPriorSigmas() { return {0.1, 0.1, 0.2, 1.0, 1.0, 1.0}; }     // :340-343
inline Sigmas AloneGpsCoordPriorSigmas() { return {0.2, 0.2, 1.57, 20.0, 20.0, 20.0}; }   // :306-309
inline Sigmas AlonePosePriorSigmas() { return {1.0e-2, 1.0e-2, 1.0e-2, 1.0e-2, 1.0e-2, 1.0e-2}; }   // :310
inline Sigmas OdomSigmas() { return {0.2, 0.2, 0.2, 1.5, 1.5, 2.0}; }                // odom_noise_model_, :92-93
inline Sigmas OdomCalibPriorSigmas() { return {0.5, 0.5, 1.5, 0.1, 0.1, 0.1}; }      // odom_tf_noise_model_ when the calibration is estimated, :85-86

// The vertices and factors, in the arrays smhip_pose_graph_optimize / smhip_pose_graph_optimize_factors take.  The frame vertex (the
// map origin in the GPS frame) is kept apart from the chain and emitted as the LAST node at every solve, so that chain vertices stay
// index-adjacent and the preconditioner keeps solving the chain exactly.  The calibration vertex (the lidar-odometer extrinsic,
// ODOM_CALIB_KEY) is kept apart likewise and emitted after the chain vertices and before the frame vertex, only when it is set.
class PoseGraph {
 public:
  struct Edge {
    int i = 0, j = 0; Matrix4d transform = Matrix4d::Identity(); Sigmas sigmas = FrameMatchSigmas(); double huber = 0;   // huber: the factor's Huber threshold, 0 = none
    bool has_information = false;                      // the edge is whitened by sqrt_information (row-major 6x6 L, information L^T L) in place
    std::array<double, 36> sqrt_information{};         // of its sigmas (include/smhip.h, "Edge information"); the sigmas stay valid and unread
  };
  // a PRIOR on vertex `index` around `pose`, a POINT between the frame vertex and vertex `index`, or a HANDEYE between vertex `index`
  // and the calibration vertex measured as `pose`
  struct Factor { int kind = SMHIP_POSE_GRAPH_FACTOR_PRIOR; int index = 0; Matrix4d pose = Matrix4d::Identity(); double lever[3] = {0, 0, 0}, point[3] = {0, 0, 0}; Sigmas sigmas = FrameMatchSigmas(); double huber = 0; };

  // :140-173.  Vertices come in index order; vertex 0 is constant.
  void AddVertex(int index, const Matrix4d& pose, const Matrix4d& transform_from_last_pose, const Sigmas& odom_noise = FrameMatchSigmas()) {
    SMHIP_CHECK(index == static_cast<int>(poses_.size()), "vertices are added in index order");
    poses_.push_back(pose);
    fixed_.push_back(index == 0 ? 1 : 0);
    if (index > 0) AddEdge(index - 1, index, transform_from_last_pose, odom_noise, 0.0);
  }
  // :127-138
  void AddLoopCloseEdge(int target_index, int source_index, const Matrix4d& transform_tgt_to_src, const Sigmas& loop_close_noise = LoopClosureSigmas(),
                        double huber = 0.0) {
    AddEdge(target_index, source_index, transform_tgt_to_src, loop_close_noise, huber);
  }
  // The same two with the matcher's own information on the edge (smhip/edge_information.h): the sigmas stay the reference's, unread
  void AddVertex(int index, const Matrix4d& pose, const Matrix4d& transform_from_last_pose, const EdgeInformation& information) {
    AddVertex(index, pose, transform_from_last_pose, FrameMatchSigmas());
    if (index > 0) SetInformation(&edges_.back(), information);
  }
  void AddLoopCloseEdge(int target_index, int source_index, const Matrix4d& transform_tgt_to_src, const EdgeInformation& information, double huber = 0.0) {
    AddEdge(target_index, source_index, transform_tgt_to_src, LoopClosureSigmas(), huber);
    SetInformation(&edges_.back(), information);
  }
  // some edge carries a square-root information
  bool HasInformation() const {
    for (const Edge& e : edges_) if (e.has_information) return true;
    return false;
  }
  // info_index and sqrt_info of smhip_pose_graph_optimize_info in the order of FlattenFactors' factors: only BETWEENs carry one
  void FlattenInformation(std::vector<int32_t>* info_index, std::vector<double>* sqrt_info) const {
    info_index->assign(static_cast<size_t>(FactorCount()), -1);
    sqrt_info->clear();
    for (size_t k = 0; k < edges_.size(); ++k) {
      if (!edges_[k].has_information) continue;
      (*info_index)[k] = static_cast<int32_t>(sqrt_info->size() / 36);
      sqrt_info->insert(sqrt_info->end(), edges_[k].sqrt_information.begin(), edges_[k].sqrt_information.end());
    }
  }
  // A vertex that is neither constant nor tied to the previous one: what SolveGpsCorrdAlone's own graph is made of (:314-320)
  int AddLooseVertex(const Matrix4d& pose) {
    poses_.push_back(pose);
    fixed_.push_back(0);
    return static_cast<int>(poses_.size()) - 1;
  }
  // Vertex `index` is held where it is from now on: a solve leaves its pose's bits (what vertex 0 of AddVertex is from the start)
  void HoldVertex(int index) {
    SMHIP_CHECK(index >= 0 && index < static_cast<int>(poses_.size()), "a held vertex exists");
    fixed_[static_cast<size_t>(index)] = 1;
  }
  void AddPriorFactor(int index, const Matrix4d& pose, const Sigmas& sigmas, double huber = 0.0) {
    SMHIP_CHECK(index >= 0 && index < static_cast<int>(poses_.size()), "a prior is on a vertex that exists");
    SMHIP_CHECK(std::isfinite(huber) && huber >= 0.0, "a Huber threshold is finite and not negative");
    Factor f;
    f.kind = SMHIP_POSE_GRAPH_FACTOR_PRIOR; f.index = index; f.pose = pose; f.sigmas = sigmas; f.huber = huber;
    factors_.push_back(f);
  }
  // The frame vertex at `pose` with a prior around it; set again, it moves and its prior with it.
  void SetFrameVertex(const Matrix4d& pose, const Sigmas& prior_sigmas) {
    has_frame_ = true; frame_pose_ = pose; frame_prior_ = pose; frame_prior_sigmas_ = prior_sigmas;
  }
  bool HasFrameVertex() const { return has_frame_; }
  const Matrix4d& FrameVertexPose() const { return frame_pose_; }
  // :238-261: frame * pose_index * lever = point, sigmas for the three rows
  void AddPointFactor(int index, const double lever[3], const double point[3], const std::array<double, 3>& sigmas3, double huber = 0.0) {
    SMHIP_CHECK(has_frame_, "a point factor needs the frame vertex");
    SMHIP_CHECK(index >= 0 && index < static_cast<int>(poses_.size()), "a point factor observes a vertex that exists");
    SMHIP_CHECK(std::isfinite(huber) && huber >= 0.0, "a Huber threshold is finite and not negative");
    Factor f;
    f.kind = SMHIP_POSE_GRAPH_FACTOR_POINT; f.index = index; f.huber = huber;
    for (int c = 0; c < 3; ++c) { f.lever[c] = lever[c]; f.point[c] = point[c]; }
    f.sigmas = {sigmas3[0], sigmas3[1], sigmas3[2], 1.0, 1.0, 1.0};            // (the last three are not read)
    factors_.push_back(f);
  }
  // The calibration vertex at `pose`, held there (the reference's prior of sigma 1e-6 as a fixed node) ...
  void SetCalibVertex(const Matrix4d& pose) { has_calib_ = true; calib_held_ = true; calib_pose_ = pose; calib_prior_ = pose; }
  // ... or free under a prior around `pose`; set again, it moves and its prior with it.
  void SetCalibVertex(const Matrix4d& pose, const Sigmas& prior_sigmas) {
    has_calib_ = true; calib_held_ = false; calib_pose_ = pose; calib_prior_ = pose; calib_prior_sigmas_ = prior_sigmas;
  }
  bool HasCalibVertex() const { return has_calib_; }
  bool CalibVertexHeld() const { return calib_held_; }
  const Matrix4d& CalibVertexPose() const { return calib_pose_; }
  // :209-224: calib^-1 * pose_index * calib = odom, six sigmas
  void AddHandEyeFactor(int index, const Matrix4d& odom, const Sigmas& sigmas = OdomSigmas(), double huber = 0.0) {
    SMHIP_CHECK(has_calib_, "a hand-eye factor needs the calibration vertex");
    SMHIP_CHECK(index >= 0 && index < static_cast<int>(poses_.size()), "a hand-eye factor observes a vertex that exists");
    SMHIP_CHECK(std::isfinite(huber) && huber >= 0.0, "a Huber threshold is finite and not negative");
    Factor f;
    f.kind = SMHIP_POSE_GRAPH_FACTOR_HANDEYE; f.index = index; f.pose = odom; f.sigmas = sigmas; f.huber = huber;
    factors_.push_back(f);
  }
  int HandEyeFactorCount() const {
    int n = 0;
    for (const Factor& f : factors_) n += f.kind == SMHIP_POSE_GRAPH_FACTOR_HANDEYE;
    return n;
  }
  bool HasFactors() const { return has_frame_ || has_calib_ || !factors_.empty(); }
  const std::vector<Factor>& Factors() const { return factors_; }
  int PointFactorCount() const {
    int n = 0;
    for (const Factor& f : factors_) n += f.kind == SMHIP_POSE_GRAPH_FACTOR_POINT;
    return n;
  }
  int NodeCount() const { return static_cast<int>(poses_.size()) + (has_calib_ ? 1 : 0) + (has_frame_ ? 1 : 0); }
  // the factors of one solve: the between-factors, the free calibration vertex's prior, the frame vertex's prior, Factors()
  int FactorCount() const { return static_cast<int>(edges_.size() + factors_.size()) + (has_calib_ && !calib_held_ ? 1 : 0) + (has_frame_ ? 1 : 0); }
  // some factor has a Huber threshold
  bool HasHuber() const {
    for (const Edge& e : edges_) if (e.huber != 0.0) return true;
    for (const Factor& f : factors_) if (f.huber != 0.0) return true;
    return false;
  }
  // the thresholds in the order of FlattenFactors' factors (the calibration and frame vertices' priors have none)
  void FlattenHuber(std::vector<double>* huber) const {
    huber->clear();
    for (const Edge& e : edges_) huber->push_back(e.huber);
    if (has_calib_ && !calib_held_) huber->push_back(0.0);
    if (has_frame_) huber->push_back(0.0);
    for (const Factor& f : factors_) huber->push_back(f.huber);
  }
  // One device solve from the current poses, which it replaces.  false (poses unchanged, the reason on stderr) when refused.  The
  // robust entry is called only when some threshold is not zero: without one the calls are those made before thresholds existed.
  // Likewise the calib entry only when a HANDEYE factor exists, and the info entry only when some edge carries an information.
  bool Optimize(smhip_handle handle, smhip_pose_graph_stats* stats = nullptr, const smhip_pose_graph_options* options = nullptr) {
    SMHIP_CHECK(handle != nullptr, "PoseGraph::Optimize needs a device handle");
    if (poses_.empty()) return true;
    if (HasInformation()) {
      std::vector<double> poses, data, sigmas, huber, sqrt_info;
      std::vector<int32_t> ij, info_index;
      std::vector<uint8_t> fixed, kinds;
      FlattenFactors(&poses, &fixed, &kinds, &ij, &data, &sigmas);
      if (HasHuber()) FlattenHuber(&huber);
      FlattenInformation(&info_index, &sqrt_info);
      const smhip_status s = smhip_pose_graph_optimize_info(handle, NodeCount(), poses.data(), fixed.data(), static_cast<int>(kinds.size()), kinds.data(),
                                                            ij.data(), data.data(), sigmas.data(), huber.empty() ? nullptr : huber.data(), info_index.data(),
                                                            sqrt_info.data(), options, stats);
      if (s != SMHIP_OK) {
        std::fprintf(stderr, "[ERROR] smhip_pose_graph_optimize_info: %s (%s)\n", smhip_status_string(s), smhip_last_error(handle));
        return false;
      }
      SetFlatNodePoses(poses);
      return true;
    }
    if (HandEyeFactorCount() > 0) {
      std::vector<double> poses, data, sigmas, huber;
      std::vector<int32_t> ij;
      std::vector<uint8_t> fixed, kinds;
      FlattenFactors(&poses, &fixed, &kinds, &ij, &data, &sigmas);
      if (HasHuber()) FlattenHuber(&huber);
      const smhip_status s = smhip_pose_graph_optimize_calib(handle, NodeCount(), poses.data(), fixed.data(), static_cast<int>(kinds.size()), kinds.data(),
                                                             ij.data(), data.data(), sigmas.data(), huber.empty() ? nullptr : huber.data(), options, stats);
      if (s != SMHIP_OK) {
        std::fprintf(stderr, "[ERROR] smhip_pose_graph_optimize_calib: %s (%s)\n", smhip_status_string(s), smhip_last_error(handle));
        return false;
      }
      SetFlatNodePoses(poses);
      return true;
    }
    if (HasHuber()) {
      std::vector<double> poses, data, sigmas, huber;
      std::vector<int32_t> ij;
      std::vector<uint8_t> fixed, kinds;
      FlattenFactors(&poses, &fixed, &kinds, &ij, &data, &sigmas);
      FlattenHuber(&huber);
      const smhip_status s = smhip_pose_graph_optimize_robust(handle, NodeCount(), poses.data(), fixed.data(), static_cast<int>(kinds.size()), kinds.data(),
                                                              ij.data(), data.data(), sigmas.data(), huber.data(), options, stats);
      if (s != SMHIP_OK) {
        std::fprintf(stderr, "[ERROR] smhip_pose_graph_optimize_robust: %s (%s)\n", smhip_status_string(s), smhip_last_error(handle));
        return false;
      }
      SetFlatNodePoses(poses);
      return true;
    }
    if (HasFactors()) {
      std::vector<double> poses, data, sigmas;
      std::vector<int32_t> ij;
      std::vector<uint8_t> fixed, kinds;
      FlattenFactors(&poses, &fixed, &kinds, &ij, &data, &sigmas);
      const smhip_status s = smhip_pose_graph_optimize_factors(handle, NodeCount(), poses.data(), fixed.data(), static_cast<int>(kinds.size()), kinds.data(),
                                                               ij.data(), data.data(), sigmas.data(), options, stats);
      if (s != SMHIP_OK) {
        std::fprintf(stderr, "[ERROR] smhip_pose_graph_optimize_factors: %s (%s)\n", smhip_status_string(s), smhip_last_error(handle));
        return false;
      }
      SetFlatNodePoses(poses);
      return true;
    }
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
  // smhip_pose_graph_last_robust for the solve Optimize ran last on `handle`, with this graph as it was then: per factor, in the
  // order of FlattenFactors, s_f, w_f and the cost term at the poses the solve ended at.  Any pointer may be null.  false (the reason
  // on stderr) when refused.
  bool Report(smhip_handle handle, std::vector<double>* norm, std::vector<double>* weight, std::vector<double>* cost = nullptr) const {
    SMHIP_CHECK(handle != nullptr, "PoseGraph::Report needs a device handle");
    const size_t m = static_cast<size_t>(FactorCount());
    if (norm) norm->assign(m, 0.0);
    if (weight) weight->assign(m, 0.0);
    if (cost) cost->assign(m, 0.0);
    const smhip_status s = smhip_pose_graph_last_robust(handle, static_cast<int>(m), norm ? norm->data() : nullptr, weight ? weight->data() : nullptr,
                                                        cost ? cost->data() : nullptr);
    if (s != SMHIP_OK) {
      std::fprintf(stderr, "[ERROR] smhip_pose_graph_last_robust: %s (%s)\n", smhip_status_string(s), smhip_last_error(handle));
      return false;
    }
    return true;
  }
  // The graph's own node numbering, which Marginals takes: the vertices 0 .. VertexCount() - 1, then the calibration vertex (when
  // set), then the frame vertex (when set); -1 for a vertex that is not there
  int CalibNodeIndex() const { return has_calib_ ? static_cast<int>(poses_.size()) : -1; }
  int FrameNodeIndex() const { return has_frame_ ? static_cast<int>(poses_.size()) + (has_calib_ ? 1 : 0) : -1; }
  // smhip_pose_graph_marginals for the solve Optimize ran last on `handle`, with this graph as it was then (what GTSAM's
  // Marginals::marginalCovariance answers in the reference): cov[q] = Sigma of nodes[q], 36 doubles row-major, in the optimiser's
  // tangent chart -- rotation first, the translation part in the node's BODY frame (WorldPositionCovariance turns it) -- relative to
  // the held vertices and the priors; zeros for a held vertex.  rows / blocks: cross blocks [H^-1]_{rows[r], nodes[q]} at
  // blocks[q * rows->size() + r], unsymmetrised (both null: none).  false (the reason on stderr) when refused.
  bool Marginals(smhip_handle handle, const std::vector<int>& nodes, std::vector<std::array<double, 36>>* cov, const std::vector<int>* rows = nullptr,
                 std::vector<std::array<double, 36>>* blocks = nullptr, smhip_pose_graph_marginals_stats* stats = nullptr,
                 const smhip_pose_graph_marginals_options* options = nullptr) const {
    SMHIP_CHECK(handle != nullptr, "PoseGraph::Marginals needs a device handle");
    SMHIP_CHECK(cov != nullptr && (rows == nullptr) == (blocks == nullptr), "cov, and rows with blocks or neither");
    const std::vector<int32_t> query(nodes.begin(), nodes.end());
    const std::vector<int32_t> row(rows ? rows->begin() : nodes.end(), rows ? rows->end() : nodes.end());
    cov->assign(query.size(), std::array<double, 36>{});
    if (blocks) blocks->assign(query.size() * row.size(), std::array<double, 36>{});
    const smhip_status s = smhip_pose_graph_marginals(handle, NodeCount(), static_cast<int>(query.size()), query.data(), cov->empty() ? nullptr : (*cov)[0].data(),
                                                      static_cast<int>(row.size()), row.empty() ? nullptr : row.data(),
                                                      blocks && !blocks->empty() ? (*blocks)[0].data() : nullptr, options, stats);
    if (s != SMHIP_OK) {
      std::fprintf(stderr, "[ERROR] smhip_pose_graph_marginals: %s (%s)\n", smhip_status_string(s), smhip_last_error(handle));
      return false;
    }
    return true;
  }
  // R_k Sigma_vv R_k^T (9 doubles, row-major) for the node `index` of the numbering above and its Sigma from Marginals
  std::array<double, 9> WorldPositionCovariance(int index, const std::array<double, 36>& cov36) const {
    SMHIP_CHECK(index >= 0 && index < NodeCount(), "a node that exists");
    const Matrix4d& X = index == CalibNodeIndex() ? calib_pose_ : index == FrameNodeIndex() ? frame_pose_ : poses_[static_cast<size_t>(index)];
    std::array<double, 9> out{};
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        double s = 0.0;
        for (int k = 0; k < 3; ++k)
          for (int l = 0; l < 3; ++l) s += X(a, k) * cov36[static_cast<size_t>(6 * (3 + k) + 3 + l)] * X(b, l);
        out[static_cast<size_t>(3 * a + b)] = s;
      }
    return out;
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
  // The arrays of smhip_pose_graph_optimize_factors: the vertices, then the calibration vertex (when set), then the frame vertex (when
  // set) as the last node; the between-factors in the order of Edges(), the calibration vertex's prior (when it is free), the frame
  // vertex's prior, then Factors() in their order.
  void FlattenFactors(std::vector<double>* poses, std::vector<uint8_t>* fixed, std::vector<uint8_t>* kinds, std::vector<int32_t>* ij, std::vector<double>* data,
                      std::vector<double>* sigmas) const {
    Flatten(poses, ij, data, sigmas);
    *fixed = fixed_;
    kinds->assign(edges_.size(), SMHIP_POSE_GRAPH_FACTOR_BETWEEN);
    const int calib = static_cast<int>(poses_.size()), frame = calib + (has_calib_ ? 1 : 0);
    auto put = [&](int kind, int i, int j, const double* d16, const Sigmas& s) {
      kinds->push_back(static_cast<uint8_t>(kind));
      ij->push_back(i); ij->push_back(j);
      data->insert(data->end(), d16, d16 + 16);
      sigmas->insert(sigmas->end(), s.begin(), s.end());
    };
    if (has_calib_) {
      poses->insert(poses->end(), calib_pose_.data(), calib_pose_.data() + 16);
      fixed->push_back(calib_held_ ? 1 : 0);
      if (!calib_held_) put(SMHIP_POSE_GRAPH_FACTOR_PRIOR, calib, calib, calib_prior_.data(), calib_prior_sigmas_);
    }
    if (has_frame_) {
      poses->insert(poses->end(), frame_pose_.data(), frame_pose_.data() + 16);
      fixed->push_back(0);
      put(SMHIP_POSE_GRAPH_FACTOR_PRIOR, frame, frame, frame_prior_.data(), frame_prior_sigmas_);
    }
    for (const Factor& f : factors_) {
      if (f.kind == SMHIP_POSE_GRAPH_FACTOR_PRIOR) {
        put(f.kind, f.index, f.index, f.pose.data(), f.sigmas);
      } else if (f.kind == SMHIP_POSE_GRAPH_FACTOR_HANDEYE) {
        put(f.kind, f.index, calib, f.pose.data(), f.sigmas);
      } else {
        double d16[16] = {f.lever[0], f.lever[1], f.lever[2], f.point[0], f.point[1], f.point[2]};
        put(f.kind, frame, f.index, d16, f.sigmas);
      }
    }
  }
  // NodeCount() poses back from a solve of FlattenFactors' arrays
  void SetFlatNodePoses(const std::vector<double>& poses) {
    SMHIP_CHECK(poses.size() == 16 * static_cast<size_t>(NodeCount()), "16 doubles per node");
    for (size_t k = 0; k < poses_.size(); ++k)
      for (int q = 0; q < 16; ++q) poses_[k].data()[q] = poses[16 * k + static_cast<size_t>(q)];
    if (has_calib_)
      for (int q = 0; q < 16; ++q) calib_pose_.data()[q] = poses[16 * poses_.size() + static_cast<size_t>(q)];
    if (has_frame_)
      for (int q = 0; q < 16; ++q) frame_pose_.data()[q] = poses[16 * (poses_.size() + (has_calib_ ? 1 : 0)) + static_cast<size_t>(q)];
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
  void AddEdge(int i, int j, const Matrix4d& transform, const Sigmas& sigmas, double huber) {
    const int n = static_cast<int>(poses_.size());
    SMHIP_CHECK(i >= 0 && j >= 0 && i < n && j < n && i != j, "an edge joins two different vertices that exist");
    SMHIP_CHECK(std::isfinite(huber) && huber >= 0.0, "a Huber threshold is finite and not negative");
    Edge e;
    e.i = i; e.j = j; e.transform = transform; e.sigmas = sigmas; e.huber = huber;
    edges_.push_back(e);
  }
  static void SetInformation(Edge* e, const EdgeInformation& information) {
    for (double v : information.sqrt_information) SMHIP_CHECK(std::isfinite(v), "a square-root information is finite");
    e->has_information = true;
    e->sqrt_information = information.sqrt_information;
  }
  std::vector<Matrix4d> poses_;
  std::vector<uint8_t> fixed_;
  std::vector<Edge> edges_;
  std::vector<Factor> factors_;
  bool has_frame_ = false;
  Matrix4d frame_pose_ = Matrix4d::Identity(), frame_prior_ = Matrix4d::Identity();
  Sigmas frame_prior_sigmas_ = GpsCoordPriorSigmas();
  bool has_calib_ = false, calib_held_ = true;
  Matrix4d calib_pose_ = Matrix4d::Identity(), calib_prior_ = Matrix4d::Identity();
  Sigmas calib_prior_sigmas_ = OdomCalibPriorSigmas();
};

struct IsamOptimizerOptions {
  int max_iterations = 50;            // of one solve (smhip_pose_graph_options)
  bool use_gps = false;               // isam_optimizer.h:61-66
  int gps_factor_init_num = 25;
  int gps_factor_sample_step = 1;
  double gps_factor_init_angle_rad = 1.6;
  bool enable_extrinsic_calib = false;   // true is refused: the tf_error point (GPS_CALIB_KEY) is not restated
  bool use_odom = false;              // isam_optimizer.h: a HANDEYE factor for every frame with an odometer reading
  bool odom_extrinsic_calib = false;  // false: the calibration vertex is held at tf_odom_lidar^-1; true: free under the prior of :85-86
  double odom_huber = 1.0;            // the Huber threshold of the odometry factors (:90-91); 0: none
  double loop_closure_huber = 0.0;    // the Huber threshold of every loop edge, and of nothing else.  0: none, the reference's
                                      // IsamOptimizer (:82-83); 1.0: the multi-trajectory optimiser's loop_closure_model_
                                      // (multi_trajectory_optimizer.cc:68-81)
  bool use_edge_information = false;  // (not in the reference) a chain edge handed in with its EdgeInformation, and a loop edge the detector
                                      // measured one for (LoopDetectorSettings::edge_information), enter the graph with it in place of
                                      // the fixed sigmas; false: every edge as before, whatever it carries
};

// One loop edge after the last solve: s_f and w_f of include/smhip.h, "Robust factors" (weight 1: taken at full weight)
struct LoopEdgeWeight {
  int target = 0, source = 0;
  double norm = 0.0, weight = 1.0;
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
  // TEST HOOK beside it: `reporter` replaces PoseGraph::Report, for the graph at the poses the solver left
  using Reporter = std::function<bool(const PoseGraph&, std::vector<double>* norm, std::vector<double>* weight)>;

  IsamOptimizer(const IsamOptimizerOptions& options, const LoopDetectorSettings& l_d_setting, smhip_handle handle)
      : loop_detector_(new LoopDetector(l_d_setting)), options_(options), handle_(handle) {
    SMHIP_CHECK(!options.enable_extrinsic_calib, "enable_extrinsic_calib is not restated: the GPS_CALIB_KEY point and the odometry calibration are out of scope");
    SMHIP_CHECK(std::isfinite(options.loop_closure_huber) && options.loop_closure_huber >= 0.0, "loop_closure_huber is finite and not negative");
    SMHIP_CHECK(std::isfinite(options.odom_huber) && options.odom_huber >= 0.0, "odom_huber is finite and not negative");
  }
  IsamOptimizer(const IsamOptimizer&) = delete;
  IsamOptimizer& operator=(const IsamOptimizer&) = delete;
  void SetSolver(Solver solver) { solver_ = std::move(solver); }
  void SetReporter(Reporter reporter) { reporter_ = std::move(reporter); }
  // TEST HOOK beside them: `marginalizer` replaces PoseGraph::Marginals, for the graph at the poses the solver left (rows and blocks
  // both null or both set, as there)
  using Marginalizer = std::function<bool(const PoseGraph&, const std::vector<int>& nodes, std::vector<std::array<double, 36>>* cov, const std::vector<int>* rows,
                                          std::vector<std::array<double, 36>>* blocks)>;
  void SetMarginalizer(Marginalizer marginalizer) { marginalizer_ = std::move(marginalizer); }
  // What the reference would ask of gtsam::Marginals (isam_optimizer.h:32), at the poses of the last solve of the main graph (not
  // SolveGpsCorrdAlone's own graph: ask before a frame that runs it or after the next solve).  Covariances are in the optimiser's
  // tangent chart, rotation first, the translation part in the vertex's body frame (PoseGraph::WorldPositionCovariance turns it),
  // and relative to vertex 0, which is held: its own is zero.  false when no solve has run, the vertex does not exist or the
  // device refused.
  bool MarginalCovariance(int frame_index, std::array<double, 36>* cov) const {
    if (frame_index < 0 || frame_index >= graph_.VertexCount()) return false;
    return NodeCovariance(frame_index, cov);
  }
  // the lidar-odometer extrinsic's (the calibration vertex; zero while it is held) and the map origin's in the GPS frame (the frame vertex)
  bool CalibCovariance(std::array<double, 36>* cov) const { return graph_.HasCalibVertex() && NodeCovariance(graph_.CalibNodeIndex(), cov); }
  bool GpsCoordCovariance(std::array<double, 36>* cov) const { return graph_.HasFrameVertex() && NodeCovariance(graph_.FrameNodeIndex(), cov); }
  // Many vertices in one call (node indices of PoseGraph's numbering)
  bool MarginalCovariances(const std::vector<int>& nodes, std::vector<std::array<double, 36>>* cov) const {
    if (!main_solved_ || !cov) return false;
    return marginalizer_ ? marginalizer_(graph_, nodes, cov, nullptr, nullptr) : graph_.Marginals(handle_, nodes, cov);
  }
  // The 12x12 joint of frames i and j, row-major, i first: the symmetrised diagonal blocks, and for the cross block the mean of
  // [H^-1]_{i,j} from j's solves and the transpose of [H^-1]_{j,i} from i's, so that the joint is symmetric to the bit
  bool JointMarginalCovariance(int i, int j, std::array<double, 144>* joint) const {
    if (!main_solved_ || !joint || i < 0 || j < 0 || i >= graph_.VertexCount() || j >= graph_.VertexCount() || i == j) return false;
    const std::vector<int> pair = {i, j};
    std::vector<std::array<double, 36>> cov, blocks;
    if (!(marginalizer_ ? marginalizer_(graph_, pair, &cov, &pair, &blocks) : graph_.Marginals(handle_, pair, &cov, &pair, &blocks))) return false;
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) {
        (*joint)[static_cast<size_t>(12 * a + b)] = cov[0][static_cast<size_t>(6 * a + b)];
        (*joint)[static_cast<size_t>(12 * (6 + a) + 6 + b)] = cov[1][static_cast<size_t>(6 * a + b)];
        // blocks[q * 2 + r] = [H^-1]_{pair[r], pair[q]}
        const double ij = 0.5 * (blocks[2][static_cast<size_t>(6 * a + b)] + blocks[1][static_cast<size_t>(6 * b + a)]);
        (*joint)[static_cast<size_t>(12 * a + 6 + b)] = ij;
        (*joint)[static_cast<size_t>(12 * (6 + b) + a)] = ij;
      }
    return true;
  }
  // tf_tracking_gps_: only its translation is used (:247-248), the antenna in the tracking frame
  void SetTransformTrackingToGps(const Matrix4d& t) { for (int c = 0; c < 3; ++c) gps_lever_[c] = t(c, 3); }
  // tf_odom_lidar_ (odom -> lidar): where the calibration vertex starts (its inverse, :153-157), so set it before the first frame;
  // RunFinalOptimazation writes the estimate back (:361-367)
  void SetTransformOdomToLidar(const Matrix4d& t) { tf_odom_lidar_ = t; }
  const Matrix4d& GetTransformOdomToLidar() const { return tf_odom_lidar_; }
  int OdomFactorCount() const { return graph_.HandEyeFactorCount(); }

  // :196-293.  `frame`: the submap as the detector sees it; `transform_from_last`: Submap::TransformFromLast(), the matched
  // transform from the previous submap (ignored for the first).  Every frame's global_pose is written back, which is what the
  // detector reads again on its next AddFrame.  false when a solve failed (the reason on stderr): the vertex and its factors stay in
  // the graph, every frame keeps the pose it had, and a later AddFrame or RunFinalOptimazation solves the whole graph again.
  bool AddFrame(const std::shared_ptr<LoopFrame>& frame, const Matrix4d& transform_from_last) {
    return AddFrame(frame, transform_from_last, nullptr);
  }
  // ... with the information of the match that gave transform_from_last (null: none); used when options.use_edge_information
  bool AddFrame(const std::shared_ptr<LoopFrame>& frame, const Matrix4d& transform_from_last, const EdgeInformation* chain_information) {
    SMHIP_CHECK(frame != nullptr, "CHECK(frame)");
    const DetectResult result = loop_detector_->AddFrame(frame, true);                          // :199
    return AddDetected(frame, transform_from_last, result, chain_information);
  }
  // TEST HOOK: the part of AddFrame after the detector (:200-292), for a detector result made by hand
  bool AddDetected(const std::shared_ptr<LoopFrame>& frame, const Matrix4d& transform_from_last, const DetectResult& result,
                   const EdgeInformation* chain_information = nullptr) {
    const int frame_index = graph_.VertexCount();
    SMHIP_CHECK(frame_index == result.current_frame_index, "CHECK_EQ(frame_index, result.current_frame_index)");   // :202
    frames_.push_back(frame);
    if (options_.use_edge_information && chain_information) graph_.AddVertex(frame_index, frame->global_pose, transform_from_last, *chain_information);
    else graph_.AddVertex(frame_index, frame->global_pose, transform_from_last, FrameMatchSigmas());  // :206-207
    if (frame_index == 0 && options_.use_odom) {                                                // :153-162
      const Matrix4d calib = RigidInverse(tf_odom_lidar_);
      if (options_.odom_extrinsic_calib) graph_.SetCalibVertex(calib, OdomCalibPriorSigmas());
      else graph_.SetCalibVertex(calib);
    }
    bool ok = Update();                                                                         // IsamUpdate of :172
    if (options_.use_odom && frame->has_odom) {                                                 // :209-224
      graph_.AddHandEyeFactor(frame_index, frame->odom, OdomSigmas(), options_.odom_huber);
      ok = Update() && ok;
    }
    if (result.close_succeed) {                                                                 // :227-236
      for (const LoopEdge& edge : result.edges) {
        loop_edge_at_.push_back(static_cast<int>(graph_.Edges().size()));
        loop_edge_searches_.push_back({edge.search_score, edge.guess_score, edge.runner_up_score, edge.search_used});
        if (options_.use_edge_information && edge.has_information) loop_edges_with_information_.push_back(edge);
        if (options_.use_edge_information && edge.has_information)
          graph_.AddLoopCloseEdge(edge.close_pair_index.first, edge.close_pair_index.second, edge.transform, edge.information, options_.loop_closure_huber);
        else
          graph_.AddLoopCloseEdge(edge.close_pair_index.first, edge.close_pair_index.second, edge.transform, LoopClosureSigmas(), options_.loop_closure_huber);
        ++loop_edges_;
      }
      ok = Update() && ok;
    }
    if (options_.use_gps && frame->has_enu) {                                                   // :264-288
      if (!calculated_first_gps_coord_) {
        if (static_cast<int>(cached_enu_.size()) < options_.gps_factor_init_num ||
            AnalyseAllFramePoseForMaxRotation() < options_.gps_factor_init_angle_rad) {
          cached_enu_[frame_index] = {frame->enu[0], frame->enu[1], frame->enu[2]};
        } else if (SolveGpsCorrdAlone()) {
          for (const auto& index_enu : cached_enu_) AddEnuFactor(index_enu.first, index_enu.second);
          ok = Update() && ok;
          calculated_first_gps_coord_ = true;
        } else {
          ok = false;
        }
      } else if (options_.gps_factor_sample_step <= 1 || frame_index % options_.gps_factor_sample_step == 0) {
        AddEnuFactor(frame_index, {frame->enu[0], frame->enu[1], frame->enu[2]});
        ok = Update() && ok;
      }
    }
    if (ok) UpdateAllPose();                                                                    // :292
    return ok;
  }
  // :175-194: the largest |acos(x_0 . x_f)| over the frames' global rotations
  double AnalyseAllFramePoseForMaxRotation() const {
    if (frames_.size() <= 1) return 0.0;
    double most = 0.0;
    const Matrix4d& first = frames_[0]->global_pose;
    for (const auto& f : frames_) {
      double dot = first(0, 0) * f->global_pose(0, 0) + first(1, 0) * f->global_pose(1, 0) + first(2, 0) * f->global_pose(2, 0);
      dot = dot > 1.0 ? 1.0 : dot < -1.0 ? -1.0 : dot;
      most = std::fmax(most, std::fabs(std::acos(dot)));
    }
    return most;
  }
  // :370-383: the frame vertex's pose -- the map origin in the GPS frame -- or identity without GPS
  Matrix4d GetGpsCoordTransform() const {
    return options_.use_gps && graph_.HasFrameVertex() ? graph_.FrameVertexPose() : Matrix4d::Identity();
  }
  int GpsFactorCount() const { return graph_.PointFactorCount(); }
  int CachedEnuCount() const { return static_cast<int>(cached_enu_.size()); }
  const smhip_pose_graph_stats& AloneStats() const { return alone_stats_; }
  bool RunFinalOptimazation() {                                                                 // :351-353, 361-367
    const bool ok = Update();
    if (ok) UpdateAllPose();
    if (ok && options_.use_odom && graph_.HasCalibVertex()) tf_odom_lidar_ = RigidInverse(graph_.CalibVertexPose());
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
  // Every loop edge, in the order added, with its norm and weight at the poses of the last solve of the main graph (one launch of
  // the report; not SolveGpsCorrdAlone's own graph, so ask before a frame that runs it or after the next solve).  Empty when there
  // is no loop edge, no solve has run yet or the report was refused.
  std::vector<LoopEdgeWeight> LoopEdgeReport() const {
    std::vector<LoopEdgeWeight> out;
    if (loop_edge_at_.empty() || !main_solved_) return out;
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
  // what the guess search of LoopDetectorSettings::guess_search found for every loop edge, in the order added (LoopEdgeReport's order);
  // zeros for an edge that was not searched
  struct LoopEdgeSearch { int search_score = 0, guess_score = 0, runner_up_score = 0; bool search_used = false; };
  const std::vector<LoopEdgeSearch>& LoopEdgeSearches() const { return loop_edge_searches_; }
  // the loop edges that entered the graph with their own information (use_edge_information), in the order added
  const std::vector<LoopEdge>& LoopEdgesWithInformation() const { return loop_edges_with_information_; }
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
    main_solved_ = ok;                                                                          // (the handle's last launch is this graph's, or none that counts)
    return ok;
  }
  void AddEnuFactor(int index, const std::array<double, 3>& enu) {                              // add_enu_factor, :238-262
    graph_.AddPointFactor(index, gps_lever_, enu.data(), GpsSigmas());
  }
  // :295-349
  bool SolveGpsCorrdAlone() {
    if (!Update()) return false;                                                                // :299-300
    PoseGraph alone;
    std::vector<int> at;
    for (const auto& index_enu : cached_enu_) {
      const Matrix4d& pose = graph_.Pose(index_enu.first);
      const int k = alone.AddLooseVertex(pose);
      alone.AddPriorFactor(k, pose, AlonePosePriorSigmas());
      at.push_back(k);
    }
    alone.SetFrameVertex(gps_coord_transform_, AloneGpsCoordPriorSigmas());
    size_t n = 0;
    for (const auto& index_enu : cached_enu_) alone.AddPointFactor(at[n++], gps_lever_, index_enu.second.data(), GpsSigmas());
    bool ok;
    if (solver_) {
      ok = solver_(&alone);
    } else {
      smhip_pose_graph_options o;
      smhip_pose_graph_default_options(&o);
      o.max_iterations = 100;                                                                   // :331
      ok = alone.Optimize(handle_, &alone_stats_, &o);
    }
    main_solved_ = false;                                                                       // the handle's last launch is the alone graph's
    if (!ok) return false;
    ++solves_;
    gps_coord_transform_ = alone.FrameVertexPose();                                             // :334
    graph_.SetFrameVertex(gps_coord_transform_, GpsCoordPriorSigmas());                         // :339-343
    return true;
  }
  bool NodeCovariance(int node, std::array<double, 36>* cov) const {
    std::vector<std::array<double, 36>> one;
    if (!cov || !MarginalCovariances({node}, &one)) return false;
    *cov = one[0];
    return true;
  }
  void UpdateAllPose() {                                                                        // :106-125
    for (size_t i = 0; i < frames_.size(); ++i) frames_[i]->global_pose = graph_.Pose(static_cast<int>(i));
  }

  std::unique_ptr<LoopDetector> loop_detector_;
  IsamOptimizerOptions options_;
  smhip_handle handle_ = nullptr;
  Solver solver_;
  Reporter reporter_;
  Marginalizer marginalizer_;
  std::vector<int> loop_edge_at_;                   // the loop edges' places in graph_.Edges()
  std::vector<LoopEdge> loop_edges_with_information_;
  std::vector<LoopEdgeSearch> loop_edge_searches_;
  bool main_solved_ = false;                        // the last solve was one of graph_, as it is now, and it succeeded
  PoseGraph graph_;
  std::vector<std::shared_ptr<LoopFrame>> frames_;
  smhip_pose_graph_stats last_stats_{}, alone_stats_{};
  int loop_edges_ = 0, solves_ = 0;
  std::map<int, std::array<double, 3>> cached_enu_;
  bool calculated_first_gps_coord_ = false;
  Matrix4d gps_coord_transform_ = Matrix4d::Identity();
  double gps_lever_[3] = {0.0, 0.0, 0.0};
  Matrix4d tf_odom_lidar_ = Matrix4d::Identity();
};

}  // namespace back_end
}  // namespace smhip

#endif  // SMHIP_POSE_GRAPH_H_
