// smhip/back_end.h -- the two other callers of the registrator boundary, restated over the GPU matchers
// (SURVEY.md §8(f) row N4).  Header-only, on top of smhip/registrator.h.
//
//   LoopDetector::CloseLoop        /root/reference/back_end/loop_detector.cc:282-318
//       guess = target_pose^-1 * source_pose with z forced to 0 (:290), a fresh IcpUsingPointMatcher per candidate
//       (:304-307), accept when GetFitnessScore() > accept_scan_match_score and store edge score = -log(score) (:308-316)
//   MapBuilder::SubmapPairMatch    /root/reference/builder/map_builder.cc:399-446
//       matcher from the configured submap_matcher_options (:408-414), guess from the first frames' global poses
//       (:427-429), NormalizeRotation(result) (:434), keep the result when score >= accepted_min_score else the guess
//       (:435-444)
//   LoopDetector::AddFrame         back_end/loop_detector.cc:48-271, with SetSearchWindow (:273-280) and CheckResult (:320-345)
//       the distance gate, the descriptor gate (matchTwoM2dpDescriptors on the frames' M2DP descriptors, smhip/m2dp.h), the
//       choice of candidate pairs, the five-state loop machine, CloseLoop per pair and CheckResult.  The candidate selection
//       (SelectLoopCandidates), the state machine (NextLoopStatus) and CheckLoopResult are free functions that touch no device.
// The pose graph that consumes the detector's edges (IsamOptimizer) is smhip/pose_graph.h, over the device optimiser; the threads
// the reference schedules all this on are host control plane and stay out.
#ifndef SMHIP_BACK_END_H_
#define SMHIP_BACK_END_H_

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <utility>
#include <thread>
#include <vector>

#include "smhip/edge_information.h"
#include "smhip/m2dp.h"
#include "smhip/registrator.h"

namespace smhip {
namespace back_end {

using registrator::Matrix4d;
using InnerCloudPtr = data::InnerPointCloudData::Ptr;

inline Matrix4d Multiply(const Matrix4d& a, const Matrix4d& b) {
  Matrix4d r;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) { double s = 0; for (int k = 0; k < 4; ++k) s += a(i, k) * b(k, j); r(i, j) = s; }
  return r;
}
// inverse of a rigid transform (what GlobalPose().inverse() is applied to)
inline Matrix4d RigidInverse(const Matrix4d& t) {
  Matrix4d r = Matrix4d::Identity();
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r(i, j) = t(j, i);
  for (int i = 0; i < 3; ++i) r(i, 3) = -(r(i, 0) * t(0, 3) + r(i, 1) * t(1, 3) + r(i, 2) * t(2, 3));
  return r;
}
// common/math.h:240-245: rotation block -> quaternion -> normalised -> rotation block
inline void NormalizeRotation(Matrix4d& t) {
  const double m00 = t(0, 0), m11 = t(1, 1), m22 = t(2, 2), tr = m00 + m11 + m22;
  double w, x, y, z;
  if (tr > 0) { double s = std::sqrt(tr + 1.0); w = 0.5 * s; s = 0.5 / s; x = (t(2, 1) - t(1, 2)) * s; y = (t(0, 2) - t(2, 0)) * s; z = (t(1, 0) - t(0, 1)) * s; }
  else {                                                         // Eigen's Quaternion(Matrix3) branch
    int i = 0; if (m11 > m00) i = 1; if (m22 > t(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double s = std::sqrt(t(i, i) - t(j, j) - t(k, k) + 1.0);
    double q[3]; q[i] = 0.5 * s; s = 0.5 / s;
    w = (t(k, j) - t(j, k)) * s; q[j] = (t(j, i) + t(i, j)) * s; q[k] = (t(k, i) + t(i, k)) * s;
    x = q[0]; y = q[1]; z = q[2];
  }
  const double n = std::sqrt(w * w + x * x + y * y + z * z);
  w /= n; x /= n; y /= n; z /= n;
  t(0, 0) = 1 - 2 * (y * y + z * z); t(0, 1) = 2 * (x * y - w * z); t(0, 2) = 2 * (x * z + w * y);
  t(1, 0) = 2 * (x * y + w * z); t(1, 1) = 1 - 2 * (x * x + z * z); t(1, 2) = 2 * (y * z - w * x);
  t(2, 0) = 2 * (x * z - w * y); t(2, 1) = 2 * (y * z + w * x); t(2, 2) = 1 - 2 * (x * x + y * y);
}

// back_end/loop_detector.h DetectResult::LoopEdge (the fields CloseLoop touches)
struct LoopEdge {
  std::pair<int, int> close_pair_index{0, 0};   // (target, source)
  Matrix4d init_guess = Matrix4d::Identity();
  Matrix4d transform = Matrix4d::Identity();
  double score = 0.0;
  bool has_information = false;                 // LoopDetectorSettings::edge_information: the accepted match's own information,
  EdgeInformation information;                  // measured at `transform` (smhip/edge_information.h)
  // LoopDetectorSettings::guess_search (not in the reference): what the correlative search around init_guess found.  init_guess stays
  // the pose-derived one; the ICP started from searched_guess when search_used is set.
  Matrix4d searched_guess = Matrix4d::Identity();
  int search_score = 0, guess_score = 0, runner_up_score = 0;    // best_score, guess_score, runner_up_score of smhip_guess_search_result
  bool search_used = false;                     // search_score > guess_score
};

inline smhip_guess_search_options DefaultGuessSearchOptions() {
  smhip_guess_search_options o;
  smhip_guess_search_default_options(&o);
  return o;
}

struct LoopDetectorSettings {                   // back_end/loop_detector_options.h:29-40
  float accept_scan_match_score = 0.75f;
  int device = 0;
  int max_points = 1 << 18;          // initial arena size; the matcher grows it to fit the clouds
  bool use_gps = false;              // (GPS in the guess is commented out in the reference, loop_detector.cc:291-300: carried, unused)
  bool use_descriptor = false;
  bool output_matched_cloud = false; // (the debug output of :232-266 is not restated: carried, unused)
  int loop_ignore_threshold = 15;
  int trying_detect_loop_count = 1;
  int nearest_history_pos_num = 4;
  float max_close_loop_distance = 25.f;
  float max_close_loop_z_distance = 1.f;
  float m2dp_match_score = 0.99f;
  bool edge_information = false;     // (not in the reference) CloseLoop measures an accepted match's 6x6 information and leaves it on the edge
  EdgeInformationOptions edge_information_options;
  // (not in the reference) CloseLoop searches a window around the pose-derived guess for the transform that puts the most source points
  // into occupied target voxels (smhip_guess_search_f32, smhip.h) and starts the ICP there when that beats the guess's own score: the
  // distance gate admits candidates 25 m apart, and a local ICP has no capture range of that size.  Off: nothing is searched.
  bool guess_search = false;
  smhip_guess_search_options guess_search_options = DefaultGuessSearchOptions();
};

// TEST HOOK: what CloseLoop calls for the search instead of scan_matcher->GuessSearch (the SetSolver pattern of smhip/pose_graph.h).
// false = the search is refused, and the pair fails.
using GuessSearcher = std::function<bool(const InnerCloudPtr& target, const InnerCloudPtr& source, const Matrix4d& guess,
                                         const smhip_guess_search_options& options, smhip_guess_search_result* out)>;

// LoopDetector::CloseLoop for one candidate pair of frames.  `scan_matcher` plays the stack matcher of :304; handing in
// one that outlives the call (the loop detector checks many candidates in a row) keeps its device arena between
// candidates -- it re-sizes itself when a cloud does not fit -- instead of allocating one per candidate.
inline bool CloseLoop(const Matrix4d& target_global_pose, const InnerCloudPtr& target_cloud, const Matrix4d& source_global_pose,
                      const InnerCloudPtr& source_cloud, const LoopDetectorSettings& settings, LoopEdge* edge,
                      registrator::IcpPointMatcherHip* scan_matcher, const GuessSearcher* searcher = nullptr) {
  Matrix4d init_guess = Multiply(RigidInverse(target_global_pose), source_global_pose);     // :287-288
  init_guess(2, 3) = 0.;                                                                     // :290 ("it is a trick")
  edge->init_guess = init_guess;
  Matrix4d start = init_guess;
  if (settings.guess_search) {
    smhip_guess_search_result found;
    const bool searched = searcher && *searcher ? (*searcher)(target_cloud, source_cloud, init_guess, settings.guess_search_options, &found)
                                                : scan_matcher->GuessSearch(target_cloud, source_cloud, init_guess, settings.guess_search_options, &found);
    if (!searched) {
      std::fprintf(stderr, "[ERROR] CloseLoop: the guess search was refused; the pair (%d, %d) fails\n", edge->close_pair_index.first, edge->close_pair_index.second);
      return false;
    }
    std::memcpy(edge->searched_guess.data(), found.transform, sizeof(double) * 16);
    edge->search_score = found.best_score; edge->guess_score = found.guess_score; edge->runner_up_score = found.runner_up_score;
    edge->search_used = found.best_score > found.guess_score;
    if (edge->search_used) start = edge->searched_guess;
  }
  scan_matcher->SetInputSource(source_cloud);
  scan_matcher->SetInputTarget(target_cloud);
  scan_matcher->Align(start, edge->transform);
  const double match_score = scan_matcher->GetFitnessScore();
  if (match_score > settings.accept_scan_match_score) {                                     // :309
    edge->score = -std::log(match_score);                                                   // :312
    if (settings.edge_information) {         // nothing is computed unless asked; a match whose information cannot be had keeps the sigmas
      AlignInformation info;
      edge->has_information = scan_matcher->GetInformation(edge->transform, &info);
      if (edge->has_information) edge->information = MakeEdgeInformation(info, settings.edge_information_options);
    }
    return true;
  }
  return false;
}
inline bool CloseLoop(const Matrix4d& target_global_pose, const InnerCloudPtr& target_cloud, const Matrix4d& source_global_pose,
                      const InnerCloudPtr& source_cloud, const LoopDetectorSettings& settings, LoopEdge* edge, const GuessSearcher* searcher = nullptr) {
  registrator::IcpPointMatcherHip scan_matcher(settings.device, settings.max_points);       // :304
  scan_matcher.InitWithOptions();
  return CloseLoop(target_global_pose, target_cloud, source_global_pose, source_cloud, settings, edge, &scan_matcher, searcher);
}

// ---- LoopDetector (back_end/loop_detector.{h,cc}) ------------------------------------------------------------------------

enum class LoopStatus : uint8_t { kNoLoop, kTryingToCloseLoop, kEnteringLoop, kContinousLoop, kLeavingLoop };   // loop_detector.h:41-47

struct DetectResult {                           // loop_detector.h:49-70
  int current_frame_index = 0;
  LoopStatus status = LoopStatus::kNoLoop;
  bool close_succeed = false;                   // is it a good loop detection result
  std::vector<LoopEdge> edges;
};

// What the detector reads of the reference's Submap: GlobalPose() / GlobalTranslation(), Cloud() and GetDescriptor().  Frames are
// shared: the detector reads their poses again on every AddFrame, since they could have been changed (:52-57).
struct LoopFrame {
  Matrix4d global_pose = Matrix4d::Identity();
  InnerCloudPtr cloud;                          // may stay empty until a CloseLoop needs it
  std::function<InnerCloudPtr()> cloud_loader;  // asked when a CloseLoop needs the cloud and `cloud` is empty (the reference's Submap::Cloud()
                                                // reloads from disk); what it returns is used for that match and not kept here
  descriptor::M2dp::Descriptor descriptor;      // read when use_descriptor is set
  bool has_enu = false;                         // FrameBase::related_enu_ (builder/frame_base.h:93-95): the GPS fix of the frame,
  double enu[3] = {0.0, 0.0, 0.0};              // already in ENU metres; read by IsamOptimizer when use_gps is set
  bool has_odom = false;                        // FrameBase::related_odom_ (HasOdom / GetRelatedOdom): the odometer's pose relative to
  Matrix4d odom = Matrix4d::Identity();         // its first reading; read by IsamOptimizer when use_odom is set
};

struct LoopCandidates {
  int loop_detection = 0;                                   // :123-127
  std::vector<std::pair<int, int>> maybe_close_pair;        // (target, source = current), :124-153
  int closest_index = -1;                                   // after the 0.4 rule, :98-100
  std::vector<int> indices_in_distance, indices_well_matched;
};

// loop_detector.cc:69-153 for the newest frame (index translations.size() - 1): the window, the xy / z gate, the closest index
// dropped at 0.4 x the distance, the descriptor gate or the copy, the step rule for nearest_history_pos_num and the closest pair
// appended.  descriptors[i] is read only when use_descriptor is set.  No device involved.
inline LoopCandidates SelectLoopCandidates(const LoopDetectorSettings& settings, const std::vector<std::array<double, 3>>& translations,
                                           const std::vector<const descriptor::M2dp::Descriptor*>& descriptors, int search_window_start,
                                           int search_window_end) {
  SMHIP_CHECK(settings.nearest_history_pos_num >= 1, "nearest_history_pos_num must be at least 1 (the step rule divides by it, :130-131)");
  LoopCandidates out;
  const int current_index = static_cast<int>(translations.size()) - 1;
  const int max_index = current_index;                                                        // :69
  const double cur_x = translations[current_index][0], cur_y = translations[current_index][1], cur_z = translations[current_index][2];
  double min_distance = std::numeric_limits<double>::max();
  int closest_index = -1;
  auto clamp = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
  int start_index = 0;
  int end_index = max_index - settings.loop_ignore_threshold;                                 // :80
  if (search_window_end >= 0 && search_window_start >= 0) {                                   // :81-84
    start_index = clamp(search_window_start, 0, max_index);
    end_index = clamp(search_window_end, 0, max_index);
  }
  for (int i = start_index; i < end_index; ++i) {                                             // :85-97
    const double dx = cur_x - translations[i][0], dy = cur_y - translations[i][1];
    const double xy_distance = std::sqrt(dx * dx + dy * dy);
    const double z_distance = std::fabs(cur_z - translations[i][2]);
    if (xy_distance <= settings.max_close_loop_distance && z_distance <= settings.max_close_loop_z_distance) {
      out.indices_in_distance.push_back(i);
      if (xy_distance < min_distance) { closest_index = i; min_distance = xy_distance; }
    }
  }
  if (min_distance >= settings.max_close_loop_distance * 0.4) closest_index = -1;             // :98-100
  out.closest_index = closest_index;

  std::vector<int>& indices_well_matched = out.indices_well_matched;
  if (!out.indices_in_distance.empty()) {                                                     // :103-121
    if (!settings.use_descriptor) {
      indices_well_matched = out.indices_in_distance;
    } else {
      for (int i : out.indices_in_distance) {
        SMHIP_CHECK(i != current_index, "CHECK_NE(i, current_index)");
        if (descriptor::matchTwoM2dpDescriptors(*descriptors[current_index], *descriptors[i]) > settings.m2dp_match_score)
          indices_well_matched.push_back(i);
      }
    }
  }
  if (!indices_well_matched.empty()) {                                                        // :126-153
    out.loop_detection = 1;
    std::sort(indices_well_matched.begin(), indices_well_matched.end());
    const size_t num = static_cast<size_t>(settings.nearest_history_pos_num);
    if (indices_well_matched.size() >= num * 2) {
      const int step = static_cast<int>(indices_well_matched.size()) / settings.nearest_history_pos_num;
      for (int i = 0; i < settings.nearest_history_pos_num; ++i) out.maybe_close_pair.push_back(std::make_pair(indices_well_matched[i * step], current_index));
    } else {
      const int size = indices_well_matched.size() > num ? settings.nearest_history_pos_num : static_cast<int>(indices_well_matched.size());
      for (int i = 0; i < size; ++i) out.maybe_close_pair.push_back(std::make_pair(indices_well_matched[i], current_index));
    }
    if (closest_index >= 0) {
      const auto closest_pair = std::make_pair(closest_index, current_index);
      if (std::find(out.maybe_close_pair.begin(), out.maybe_close_pair.end(), closest_pair) == out.maybe_close_pair.end())
        out.maybe_close_pair.push_back(closest_pair);
    }
  }
  return out;
}

// the loop machine, loop_detector.cc:155-206: the status after a frame with (1) or without (0) a detection
inline LoopStatus NextLoopStatus(LoopStatus current_status, int loop_detection, const LoopDetectorSettings& settings,
                                 int* accumulate_loop_detected_count) {
  switch (current_status) {
    case LoopStatus::kNoLoop:
      *accumulate_loop_detected_count = 0;
      if (loop_detection == 1) {
        current_status = LoopStatus::kTryingToCloseLoop;
        ++*accumulate_loop_detected_count;
        if (*accumulate_loop_detected_count >= settings.trying_detect_loop_count) current_status = LoopStatus::kEnteringLoop;
      }
      break;
    case LoopStatus::kTryingToCloseLoop:
      if (loop_detection == 1) {
        ++*accumulate_loop_detected_count;
        if (*accumulate_loop_detected_count >= settings.trying_detect_loop_count) current_status = LoopStatus::kEnteringLoop;
      } else if (loop_detection == 0) {
        current_status = LoopStatus::kNoLoop;
      }
      break;
    case LoopStatus::kEnteringLoop:
      if (loop_detection == 0) current_status = LoopStatus::kTryingToCloseLoop;
      else if (loop_detection == 1) current_status = LoopStatus::kContinousLoop;
      break;
    case LoopStatus::kContinousLoop:
      if (loop_detection == 0) { current_status = LoopStatus::kLeavingLoop; *accumulate_loop_detected_count = 0; }
      break;
    case LoopStatus::kLeavingLoop:
      if (loop_detection == 0) current_status = LoopStatus::kNoLoop;
      else if (loop_detection == 1) current_status = LoopStatus::kTryingToCloseLoop;
      break;
    default:
      break;
  }
  return current_status;
}

// common::RotationMatrixToEulerAngles (common/math.h:108-127) of a transform's rotation block
inline void RotationMatrixToEulerAngles(const Matrix4d& R, double eulers[3]) {
  const double sy = std::sqrt(R(0, 0) * R(0, 0) + R(1, 0) * R(1, 0));
  if (!(sy < 1e-6)) {
    eulers[0] = std::atan2(R(2, 1), R(2, 2)); eulers[1] = std::atan2(-R(2, 0), sy); eulers[2] = std::atan2(R(1, 0), R(0, 0));
  } else {
    eulers[0] = std::atan2(-R(1, 2), R(1, 1)); eulers[1] = std::atan2(-R(2, 0), sy); eulers[2] = 0;
  }
}

// LoopDetector::CheckResult, loop_detector.cc:320-345: more than one edge, and every edge puts the source within 0.25 m and
// 0.02 rad (norm of the Euler angles) of where the first edge puts it.  target_poses[k] = GlobalPose() of edge k's target.
inline bool CheckLoopResult(const std::vector<LoopEdge>& edges, const std::vector<Matrix4d>& target_poses) {
  if (edges.size() <= 1) return false;
  const Matrix4d first_source_pose = Multiply(target_poses[0], edges[0].transform);
  for (size_t i = 1; i < edges.size(); ++i) {
    const Matrix4d source_edge = Multiply(target_poses[i], edges[i].transform);
    const Matrix4d diff = Multiply(RigidInverse(first_source_pose), source_edge);
    const double trans_diff = std::sqrt(diff(0, 3) * diff(0, 3) + diff(1, 3) * diff(1, 3) + diff(2, 3) * diff(2, 3));
    double e[3];
    RotationMatrixToEulerAngles(diff, e);
    const double rotation_diff = std::sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    if (trans_diff > 0.25 || rotation_diff > 0.02) return false;
  }
  return true;
}

class LoopDetector {
 public:
  explicit LoopDetector(const LoopDetectorSettings& l_d_settings) : settings_(l_d_settings) {}
  LoopDetector(const LoopDetector&) = delete;
  LoopDetector& operator=(const LoopDetector&) = delete;

  // loop_detector.cc:48-271
  DetectResult AddFrame(const std::shared_ptr<LoopFrame>& frame, bool do_loop_detect = true) {
    SMHIP_CHECK(frame != nullptr, "null frame");
    all_frames_.push_back(frame);
    // Update all positions since they could have been changed.
    all_frames_translation_.emplace_back();
    for (size_t i = 0; i < all_frames_.size(); ++i)
      all_frames_translation_[i] = {all_frames_[i]->global_pose(0, 3), all_frames_[i]->global_pose(1, 3), all_frames_[i]->global_pose(2, 3)};
    const int current_index = static_cast<int>(all_frames_.size()) - 1;

    DetectResult result;
    result.status = current_status_;
    result.current_frame_index = current_index;
    if (!do_loop_detect || all_frames_.size() <= static_cast<size_t>(settings_.loop_ignore_threshold)) return result;   // :64-67

    std::vector<const descriptor::M2dp::Descriptor*> descriptors(all_frames_.size());
    for (size_t i = 0; i < all_frames_.size(); ++i) descriptors[i] = &all_frames_[i]->descriptor;
    last_candidates_ = SelectLoopCandidates(settings_, all_frames_translation_, descriptors, search_window_start_, search_window_end_);
    loop_detection_ = last_candidates_.loop_detection;
    const std::vector<std::pair<int, int>>& maybe_close_pair = last_candidates_.maybe_close_pair;

    current_status_ = NextLoopStatus(current_status_, loop_detection_, settings_, &accumulate_loop_detected_count_);

    if (current_status_ == LoopStatus::kContinousLoop) {                                       // :213-268
      SMHIP_CHECK(!maybe_close_pair.empty(), "CHECK(!maybe_close_pair.empty())");
      // (the reference hands the pairs to a tbb::task_group and collects the edges in the order they finish; here they run one
      // after the other through one matcher that keeps its device arena, and the edges come in the pairs' order)
      for (const auto& p : maybe_close_pair) {
        LoopEdge loop_edge;
        loop_edge.close_pair_index = p;
        if (CloseLoopPair(&loop_edge)) result.edges.push_back(loop_edge);
      }
      if (!result.edges.empty()) result.close_succeed = CheckResult(result);
    }
    return result;
  }

  void SetSearchWindow(const int start_index, const int end_index) {                           // :273-280
    SMHIP_CHECK(start_index >= 0, "CHECK_GE(start_index, 0)");
    SMHIP_CHECK(end_index >= 0, "CHECK_GE(end_index, 0)");
    SMHIP_CHECK(end_index >= start_index, "CHECK_GE(end_index, start_index)");
    search_window_start_ = start_index;
    search_window_end_ = end_index;
  }
  const std::vector<std::shared_ptr<LoopFrame>>& GetFrames() const { return all_frames_; }
  std::pair<int, int> SearchWindow() const { return {search_window_start_, search_window_end_}; }    // (-1, -1): none set
  LoopStatus Status() const { return current_status_; }
  // TEST HOOKS: `searcher` replaces the device guess search of CloseLoopPair (settings.guess_search), `matcher` the scan matcher it
  // would create on first use
  void SetGuessSearcher(GuessSearcher searcher) { guess_searcher_ = std::move(searcher); }
  void SetScanMatcher(std::unique_ptr<registrator::IcpPointMatcherHip> matcher) { scan_matcher_ = std::move(matcher); }
  // what the last AddFrame that searched selected (for inspection and tests)
  const LoopCandidates& LastCandidates() const { return last_candidates_; }

  bool CheckResult(const DetectResult& result) const {                                         // :320-345
    std::vector<Matrix4d> target_poses;
    for (const LoopEdge& e : result.edges) target_poses.push_back(all_frames_.at(static_cast<size_t>(e.close_pair_index.first))->global_pose);
    return CheckLoopResult(result.edges, target_poses);
  }

 protected:
  bool CloseLoopPair(LoopEdge* edge) {                                                         // :282-318
    const size_t target_id = static_cast<size_t>(edge->close_pair_index.first), source_id = static_cast<size_t>(edge->close_pair_index.second);
    SMHIP_CHECK(all_frames_.size() > target_id && all_frames_.size() > source_id, "CHECK(all_frames_.size() > target_id && ... > source_id)");
    const InnerCloudPtr target_cloud = FrameCloud(*all_frames_[target_id]), source_cloud = FrameCloud(*all_frames_[source_id]);
    SMHIP_CHECK(target_cloud && source_cloud, "a frame of a candidate pair has no cloud");
    if (!scan_matcher_) {
      scan_matcher_.reset(new registrator::IcpPointMatcherHip(settings_.device, settings_.max_points));
      scan_matcher_->InitWithOptions();
    }
    return CloseLoop(all_frames_[target_id]->global_pose, target_cloud, all_frames_[source_id]->global_pose, source_cloud, settings_, edge,
                     scan_matcher_.get(), &guess_searcher_);
  }
  static InnerCloudPtr FrameCloud(const LoopFrame& frame) {
    if (frame.cloud) return frame.cloud;
    return frame.cloud_loader ? frame.cloud_loader() : InnerCloudPtr();
  }

 private:
  std::vector<std::shared_ptr<LoopFrame>> all_frames_;
  std::vector<std::array<double, 3>> all_frames_translation_;
  int loop_detection_ = 0;
  int accumulate_loop_detected_count_ = 0;
  LoopStatus current_status_ = LoopStatus::kNoLoop;
  LoopDetectorSettings settings_;
  int search_window_start_ = -1;
  int search_window_end_ = -1;
  LoopCandidates last_candidates_;
  std::unique_ptr<registrator::IcpPointMatcherHip> scan_matcher_;
  GuessSearcher guess_searcher_;
};

struct SubmapPairMatchResult {
  Matrix4d transform_to_next = Matrix4d::Identity();   // what SetMatchedTransformedToNext receives
  Matrix4d guess = Matrix4d::Identity();
  double match_score = 0.0;                            // source_submap->match_score_to_previous_submap_
  bool accepted = false;
  bool has_information = false;                        // SubmapPairMatchBatch with `information_options`: an accepted pair's own information,
  EdgeInformation information;                         // measured at transform_to_next (smhip/edge_information.h)
};

// MapBuilder::SubmapPairMatch for one (source, target) pair of submaps
// `options` = back_end_options.submap_matcher_options (type, accepted_min_score, <registrator_options> text)
inline SubmapPairMatchResult SubmapPairMatch(const registrator::MatcherOptions& options, const InnerCloudPtr& source_submap_cloud,
                                             const Matrix4d& source_first_frame_pose, const InnerCloudPtr& target_submap_cloud,
                                             const Matrix4d& target_first_frame_pose) {
  SubmapPairMatchResult out;
  auto matcher = registrator::CreateMatcher(options, false);                        // :408-414
  SMHIP_CHECK(matcher != nullptr, "CreateMatcher returned null");
  if (matcher->GetType() == registrator::kFastIcp && !target_submap_cloud->GetEigenCloud()->HasNormals())
    target_submap_cloud->CalculateNormals();                                                 // Submap::Cloud() carries normals (submap.cc:161)
  matcher->SetInputSource(source_submap_cloud);
  matcher->SetInputTarget(target_submap_cloud);
  Matrix4d result = Matrix4d::Identity();
  out.guess = Multiply(RigidInverse(target_first_frame_pose), source_first_frame_pose);     // :427-429
  matcher->Align(out.guess, result);
  NormalizeRotation(result);                                                                 // :434
  out.match_score = matcher->GetFitnessScore();
  if (out.match_score >= options.accepted_min_score) { out.transform_to_next = result; out.accepted = true; }   // :437-439
  else { out.transform_to_next = out.guess; out.accepted = false; }                           // :440-444
  return out;
}

// The back end runs up to six SubmapPairMatch tasks at once on its thread pool (map_builder.cc:655, 706-708), each with
// its own matcher.  On the device the same six pairs are ONE batch: `matcher` (from CreateMatcher with the configured
// submap_matcher_options; kept by the caller between batches, so no arena is allocated per pair) aligns all of them in
// one launch sequence through its pair slots.  Matcher types without a batched form fall back to one Align per pair on
// that same matcher.  Results are those of SubmapPairMatch pair by pair.
struct SubmapPairJob {
  InnerCloudPtr source_submap_cloud, target_submap_cloud;
  Matrix4d source_first_frame_pose = Matrix4d::Identity(), target_first_frame_pose = Matrix4d::Identity();
};

// information_options (null: nothing is computed): with an IcpFast matcher every accepted pair's result also carries the
// information of its match, all of them measured in ONE further call on the batch's resident clouds.  Where the pairs were aligned
// one by one (no batch was taken), an IcpFast or IcpPointMatcher measures each pair after its Align.  A matcher that cannot measure
// (the batch form of IcpPointMatcher, Ndt, NdtWithGicp) says so on stderr, once, and its edges keep the fixed sigmas.
inline std::vector<SubmapPairMatchResult> SubmapPairMatchBatch(const registrator::MatcherOptions& options,
                                                               const std::shared_ptr<registrator::Interface>& matcher,
                                                               const std::vector<SubmapPairJob>& jobs,
                                                               const EdgeInformationOptions* information_options = nullptr) {
  SMHIP_CHECK(matcher != nullptr, "CreateMatcher returned null");
  const size_t K = jobs.size();
  std::vector<SubmapPairMatchResult> out(K);
  if (K == 0) return out;
  std::vector<InnerCloudPtr> src(K), tgt(K);
  std::vector<Matrix4d> guess(K), result;
  std::vector<double> score;
  for (size_t k = 0; k < K; ++k) {
    src[k] = jobs[k].source_submap_cloud; tgt[k] = jobs[k].target_submap_cloud;
    if (matcher->GetType() == registrator::kFastIcp && !tgt[k]->GetEigenCloud()->HasNormals()) tgt[k]->CalculateNormals();   // submap.cc:161
    guess[k] = Multiply(RigidInverse(jobs[k].target_first_frame_pose), jobs[k].source_first_frame_pose);                     // :427-429
    out[k].guess = guess[k];
  }
  bool batched = false;
  if (auto* fast = dynamic_cast<registrator::IcpFastHip*>(matcher.get())) batched = fast->AlignBatch(src, tgt, guess, &result, &score);
  else if (auto* pm = dynamic_cast<registrator::IcpPointMatcherHip*>(matcher.get())) batched = pm->AlignBatch(src, tgt, guess, &result, &score);
  else if (auto* ndt = dynamic_cast<registrator::NdtHip*>(matcher.get())) batched = ndt->AlignBatch(src, tgt, guess, &result, &score);   // lock-step Newton
  else if (auto* ng = dynamic_cast<registrator::NdtGicpHip*>(matcher.get())) batched = ng->AlignBatch(src, tgt, guess, &result, &score);   // lock-step NDT + BFGS
  std::vector<AlignInformation> single_info(information_options ? K : 0);
  std::vector<uint8_t> single_has(single_info.size(), 0);
  bool can_measure = false;
  if (!batched) {
    result.assign(guess.begin(), guess.end());
    score.assign(K, 0.0);
    auto* one_fast = dynamic_cast<registrator::IcpFastHip*>(matcher.get());
    auto* one_pm = dynamic_cast<registrator::IcpPointMatcherHip*>(matcher.get());
    can_measure = one_fast || one_pm;
    for (size_t k = 0; k < K; ++k) {
      matcher->SetInputSource(src[k]);
      matcher->SetInputTarget(tgt[k]);
      matcher->Align(guess[k], result[k]);
      score[k] = matcher->GetFitnessScore();
      if (information_options && can_measure && score[k] >= options.accepted_min_score) {   // while the pair is still on the device
        Matrix4d at = result[k];
        NormalizeRotation(at);
        single_has[k] = (one_fast ? one_fast->GetInformation(at, &single_info[k]) : one_pm->GetInformation(at, &single_info[k])) ? 1 : 0;
      }
    }
  }
  for (size_t k = 0; k < K; ++k) {
    NormalizeRotation(result[k]);                                                              // :434
    out[k].match_score = score[k];
    if (score[k] >= options.accepted_min_score) { out[k].transform_to_next = result[k]; out[k].accepted = true; }   // :437-439
    else { out[k].transform_to_next = out[k].guess; out[k].accepted = false; }                 // :440-444
  }
  auto* fast = dynamic_cast<registrator::IcpFastHip*>(matcher.get());
  if (information_options && !batched) {
    for (size_t k = 0; k < K; ++k)
      if (out[k].accepted && single_has[k]) { out[k].has_information = true; out[k].information = MakeEdgeInformation(single_info[k], *information_options); }
  }
  if (information_options && !(batched ? fast != nullptr : can_measure)) {
    static bool said = false;
    if (!said) std::fprintf(stderr, "[WARN] SubmapPairMatchBatch: this matcher cannot measure the information of its matches here; the edges keep the fixed sigmas\n");
    said = true;
  }
  if (information_options && batched && fast) {
    std::vector<Matrix4d> at(K);
    for (size_t k = 0; k < K; ++k) at[k] = out[k].transform_to_next;
    std::vector<AlignInformation> info;
    std::vector<uint8_t> has;
    if (fast->GetInformationBatch(at, &info, &has))
      for (size_t k = 0; k < K; ++k)
        if (out[k].accepted && has[k]) { out[k].has_information = true; out[k].information = MakeEdgeInformation(info[k], *information_options); }
  }
  return out;
}

// The reference's own form of concurrency (every matcher also has a batched form above): the back end's thread
// pool runs up to six SubmapPairMatch tasks at once, each with a matcher of its own (map_builder.cc:399-446, 655, 706-708).
// Here: `concurrency` matchers created once and kept between batches (every one owns a device arena and a HIP stream), the
// jobs dealt to them round-robin, one host thread per matcher -- the GPU runs the matchers' streams side by side, so the
// launch latencies, read-backs and host-side Newton / BFGS steps of one pair hide behind the kernels of the others.
// Results are those of SubmapPairMatch pair by pair (every pair runs exactly the single-pair code on its own handle).
class SubmapMatcherPool {
 public:
  SubmapMatcherPool(const registrator::MatcherOptions& options, int concurrency = 6) : options_(options) {
    for (int k = 0; k < std::max(1, concurrency); ++k) {
      auto m = registrator::CreateMatcher(options, false);
      SMHIP_CHECK(m != nullptr, "CreateMatcher returned null");
      // members of a pool align at the same time: IcpFast's single-pair cooperative launch would queue them one behind the other
      if (concurrency > 1 && options.type == registrator::kFastIcp) {
        m->InitWithXml("<param name=\"single_launch\"> 0 </param>");
        m->InitWithOptions();
      }
      matchers_.push_back(m);
    }
  }
  int concurrency() const { return static_cast<int>(matchers_.size()); }
  std::vector<SubmapPairMatchResult> Match(const std::vector<SubmapPairJob>& jobs) {
    const size_t K = jobs.size();
    std::vector<SubmapPairMatchResult> out(K);
    // CalculateNormals mutates a cloud: done up front on this thread, once per cloud (two jobs may share a target)
    if (options_.type == registrator::kFastIcp)
      for (const auto& j : jobs)
        if (!j.target_submap_cloud->GetEigenCloud()->HasNormals()) j.target_submap_cloud->CalculateNormals();
    std::vector<std::thread> workers;
    const size_t C = std::min(matchers_.size(), K);
    for (size_t t = 0; t < C; ++t) {
      workers.emplace_back([&, t] {
        registrator::Interface& m = *matchers_[t];
        for (size_t k = t; k < K; k += C) {
          SubmapPairMatchResult& r = out[k];
          m.SetInputSource(jobs[k].source_submap_cloud);
          m.SetInputTarget(jobs[k].target_submap_cloud);
          Matrix4d result = Matrix4d::Identity();
          r.guess = Multiply(RigidInverse(jobs[k].target_first_frame_pose), jobs[k].source_first_frame_pose);   // :427-429
          m.Align(r.guess, result);
          NormalizeRotation(result);                                                                           // :434
          r.match_score = m.GetFitnessScore();
          if (r.match_score >= options_.accepted_min_score) { r.transform_to_next = result; r.accepted = true; }   // :437-439
          else { r.transform_to_next = r.guess; r.accepted = false; }                                               // :440-444
        }
      });
    }
    for (auto& w : workers) w.join();
    return out;
  }

 private:
  registrator::MatcherOptions options_;
  std::vector<std::shared_ptr<registrator::Interface>> matchers_;
};

}  // namespace back_end
}  // namespace smhip

#endif  // SMHIP_BACK_END_H_
