// smhip/submap.h -- static_map::Submap's cloud and the matching of consecutive submaps, restated over the device build
// (smhip_submap_build_f32) and the back end's batch.  Header-only, on top of smhip/back_end.h and smhip/filters.h.
//
//   Submap::InsertFrame            the reference's builder/submap.cc:76-163
//       the first frame's global pose becomes the submap's pose and its local pose the identity (:80-85); every other
//       frame gets local pose = submap pose^-1 * frame pose (:87); the submap is full after frame_count frames (:94-96);
//       a full submap's frames are moved by their local poses into the first frame's coordinates and concatenated
//       (:115-124), passed through a VoxelGrid of voxel_size when enable_voxel_filter is set (:144-158), and the result
//       goes through CalculateNormals (:160-161)
//   MapBuilder::SubmapPairMatch    builder/map_builder.cc:399-446 (source = the later submap, target = the earlier one,
//       guess from the first frames' global poses, :426-428), for every pair of consecutive submaps
//
// What differs from the reference, on purpose:
//   * InsertFrame keeps the books only; the cloud is built on the device the first time it is asked for (Cloud(), or the
//     device forms that hand it to a matcher without a download), so a program without a device can still fill submaps.
//   * The voxel size reaches the filter as the reference's text would carry it: std::to_string(voxel_size), six decimals
//     (:148-154), parsed back by the filter's own parameter parse.  The reference's text names the filter "RandomSampler"
//     (:149), which its VoxelGrid::InitFromXmlText refuses before reading a parameter (filter_interface.cc:32-35), so there
//     the filter runs with its default of 0.1 whatever the option says; here the option takes effect, and at the default
//     0.1 the two agree.
//   * enable_inner_mrvm (its result is discarded, :100-113), the commented-out random sampling (:134-142), enable_check
//     and the saving to disk are not restated and have no option here.
#ifndef SMHIP_SUBMAP_H_
#define SMHIP_SUBMAP_H_

#include <cmath>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "smhip/back_end.h"
#include "smhip/filters.h"
#include "smhip/m2dp.h"

namespace smhip {
namespace builder {

using registrator::Matrix4d;
using InnerCloudPtr = data::InnerPointCloudData::Ptr;
using DeviceContext = pre_processers::filter::DeviceContext;

struct SubmapOptions {                       // builder/submap_options.h:30-38
  int32_t frame_count = 5;
  bool enable_voxel_filter = false;
  float voxel_size = 0.1f;
};

// the voxel size after its trip through the filter's XML text (submap.cc:148-154); no device involved
inline float TextVoxelSize(float voxel_size) {
  pre_processers::filter::VoxelGrid voxel_filter;
  const std::string text = "<filter name=\"VoxelGrid\" ><param type=\"1\" name=\"voxel_size\">" + std::to_string(voxel_size) +
                           "</param></filter>";
  voxel_filter.InitFromXmlText(text.c_str());
  return voxel_filter.Desc().p[0];
}

class Submap {
 public:
  explicit Submap(const SubmapOptions& options = SubmapOptions()) : options_(options) {
    SMHIP_CHECK(options_.frame_count >= 1, "frame_count must be at least 1");
  }

  // submap.cc:76-96.  `cloud`: the frame's points in the sensor frame; `global_pose`: the frame's pose.
  void InsertFrame(const data::InnerCloudType::Ptr& cloud, const Matrix4d& global_pose) {
    SMHIP_CHECK(cloud != nullptr, "CHECK(frame != nullptr)");
    SMHIP_CHECK(!full_, "CHECK(!full_): InsertFrame on a full submap");                               // :78
    if (frames_.empty()) {
      global_pose_ = global_pose;                                                                     // :83
      local_poses_.push_back(Matrix4d::Identity());                                                   // :84
    } else {
      local_poses_.push_back(back_end::Multiply(back_end::RigidInverse(global_pose_), global_pose));  // :87
    }
    frames_.push_back(cloud);
    frame_global_poses_.push_back(global_pose);
    if (static_cast<int32_t>(frames_.size()) == options_.frame_count) full_ = true;                   // :94-96
  }
  bool Full() const { return full_; }
  int FrameCount() const { return static_cast<int>(frames_.size()); }
  const Matrix4d& LocalPose(int i) const { return local_poses_.at(static_cast<size_t>(i)); }
  // GetFrames()[0]->GlobalPose(), what SubmapPairMatch builds its guess from (map_builder.cc:426-428)
  const Matrix4d& FirstFramePose() const { return global_pose_; }
  // Submap::GlobalPose / SetGlobalPose (what the pose graph reads and writes, isam_optimizer.cc:106-125) and
  // UpdateInnerFramePose, submap.cc:268-274: every frame's global pose = submap pose * local pose.  Until it is called the frames
  // keep the poses they were inserted with.
  const Matrix4d& GlobalPose() const { return global_pose_; }
  void SetGlobalPose(const Matrix4d& pose) { global_pose_ = pose; }
  void UpdateInnerFramePose() {
    for (size_t i = 0; i < frame_global_poses_.size(); ++i) frame_global_poses_[i] = back_end::Multiply(global_pose_, local_poses_[i]);
  }
  const Matrix4d& FrameGlobalPose(int i) const { return frame_global_poses_.at(static_cast<size_t>(i)); }
  const SubmapOptions& Options() const { return options_; }
  // rows of all frames together: what a handle must have room for
  int TotalPoints() const {
    size_t n = 0;
    for (const auto& f : frames_) n += f->points.size();
    return static_cast<int>(n);
  }
  // 0 when the voxel filter is off or the cloud is empty (:144), else the size as the filter receives it
  float DeviceVoxelSize() const { return options_.enable_voxel_filter ? TextVoxelSize(options_.voxel_size) : 0.f; }

  // The cloud of a full submap on `handle`'s device, left resident in the handle's filter workspace (smhip_filter_get_output,
  // smhip_filter_output_to_source and smhip_filter_output_to_target read it).  Returns its size, 0 when the device refused.
  int BuildResident(smhip_handle handle) const {
    SMHIP_CHECK(full_, "the submap is not full: it has no cloud yet");
    const int K = static_cast<int>(frames_.size());
    std::vector<const float*> rows(static_cast<size_t>(K));
    std::vector<int> n(static_cast<size_t>(K));
    std::vector<double> poses(16 * static_cast<size_t>(K));
    static_assert(sizeof(data::InnerPointType) == 5 * sizeof(float), "InnerPointType rows are five floats");
    for (int k = 0; k < K; ++k) {
      n[k] = static_cast<int>(frames_[k]->points.size());
      rows[k] = n[k] > 0 ? &frames_[k]->points[0].x : nullptr;
      for (int q = 0; q < 16; ++q) poses[16 * static_cast<size_t>(k) + q] = local_poses_[k].data()[q];
    }
    int m = 0;
    const smhip_status s = smhip_submap_build_f32(handle, K, rows.data(), 5, n.data(), poses.data(), DeviceVoxelSize(), &m);
    if (s != SMHIP_OK) {
      std::fprintf(stderr, "[ERROR] smhip_submap_build_f32: %s (%s)\n", smhip_status_string(s), smhip_last_error(handle));
      return 0;
    }
    return m;
  }

  // Submap::Cloud(): the InnerPointCloudData of submap.cc:160-161, normals calculated.  Built on `context`'s device on the
  // first call (the process-wide default context when none is given) and kept.
  InnerCloudPtr Cloud(const std::shared_ptr<DeviceContext>& context = nullptr) {
    if (cloud_) return cloud_;
    const std::shared_ptr<DeviceContext> c = context ? context : DeviceContext::Default();
    const int m = BuildResident(c->handle());
    SMHIP_CHECK(m > 0, "the submap's cloud could not be built on the device");
    std::vector<data::InnerPointType> rows(static_cast<size_t>(m));
    const smhip_status s = smhip_filter_get_output(c->handle(), &rows[0].x, nullptr, m);
    SMHIP_CHECK(s == SMHIP_OK, "smhip_filter_get_output failed");
    cloud_.reset(new data::InnerPointCloudData(rows));
    cloud_->CalculateNormals();                                                                       // :161
    return cloud_;
  }

  // FrameBase::CalculateDescriptor / GetDescriptor / SetDescriptor (builder/frame_base.cc:99-112) for the submap's cloud: built
  // on `context`'s device (the process-wide default context when none is given) and described where it lies (descriptor::M2dp
  // with its defaults, smhip/m2dp.h), without a download.  false (and the descriptor left as it was) when none was got.
  bool CalculateDescriptor(const std::shared_ptr<DeviceContext>& context = nullptr) {
    const std::shared_ptr<DeviceContext> c = context ? context : DeviceContext::Default();
    descriptor::M2dp m2dp;
    if (BuildResident(c->handle()) > 0 && m2dp.setInputCloudResident(c->handle())) {
      descriptor_ = m2dp.getFinalDescriptor();
      return true;
    }
    std::fprintf(stderr, "[ERROR] did not get a descriptor for the frame.\n");
    return false;
  }
  descriptor::M2dp::Descriptor GetDescriptor() const { return descriptor_; }
  void SetDescriptor(const descriptor::M2dp::Descriptor& d) { descriptor_ = d; }
  // FrameBase::SetRelatedGpsInENU / GetRelatedGpsInENU / HasGps (builder/frame_base.h:60-66, 93-95): the fix of the submap's first
  // frame, the frame whose pose is the submap's global pose, in ENU metres
  void SetRelatedGpsInENU(double east, double north, double up) { enu_[0] = east; enu_[1] = north; enu_[2] = up; has_gps_ = true; }
  const double* GetRelatedGpsInENU() const { return enu_; }
  bool HasGps() const { return has_gps_; }

  // Device forms: the cloud is built on the matcher's own handle and becomes its source / its CalculateNormals target without
  // a download.  Return the number of points the matcher holds (0 when the device refused; Align then fails loudly).
  int ToSource(registrator::IcpFastHip* matcher) const {
    return matcher->SetInputSourceResident(TotalPoints(), [this](smhip_handle h) { return BuildResident(h) > 0; });
  }
  int ToTarget(registrator::IcpFastHip* matcher) const {
    return matcher->SetInputTargetResident(TotalPoints(), [this](smhip_handle h) { return BuildResident(h) > 0; });
  }

 private:
  SubmapOptions options_;
  bool full_ = false;
  Matrix4d global_pose_ = Matrix4d::Identity();
  std::vector<data::InnerCloudType::Ptr> frames_;
  std::vector<Matrix4d> local_poses_, frame_global_poses_;
  InnerCloudPtr cloud_;
  descriptor::M2dp::Descriptor descriptor_;
  bool has_gps_ = false;
  double enu_[3] = {0.0, 0.0, 0.0};
};

// The pairs ConnectSubmaps matches, in its order: for k = 0, 1, ... source = submap k + 1 on target = submap k
// (map_builder.cc:399-404 with the indices the builder passes for neighbours), guess = target first pose^-1 * source first
// pose (:426-428).  Submaps that are not full have no cloud (submap.cc:98) and take part in no pair.  No device involved.
struct SubmapPair {
  int source = 0, target = 0;
  Matrix4d guess = Matrix4d::Identity();
};
inline std::vector<SubmapPair> ConsecutivePairs(const std::vector<std::shared_ptr<Submap>>& submaps) {
  std::vector<SubmapPair> pairs;
  for (size_t k = 0; k + 1 < submaps.size(); ++k) {
    if (!submaps[k]->Full() || !submaps[k + 1]->Full()) continue;
    SubmapPair p;
    p.source = static_cast<int>(k + 1); p.target = static_cast<int>(k);
    p.guess = back_end::Multiply(back_end::RigidInverse(submaps[k]->FirstFramePose()), submaps[k + 1]->FirstFramePose());
    pairs.push_back(p);
  }
  return pairs;
}

// MapBuilder::SubmapPairMatch for every pair of consecutive submaps, as ONE batch on `matcher` (back_end::SubmapPairMatchBatch):
// result k belongs to ConsecutivePairs(submaps)[k]; transform_to_next is what submap `target` would keep
// (SetMatchedTransformedToNext: the match when its score reaches accepted_min_score, else the guess, :436-444).  With
// information_options every accepted pair's result also carries the information of its match (smhip/edge_information.h).
inline std::vector<back_end::SubmapPairMatchResult> ConnectSubmaps(const registrator::MatcherOptions& options,
                                                                   const std::shared_ptr<registrator::Interface>& matcher,
                                                                   const std::vector<std::shared_ptr<Submap>>& submaps,
                                                                   const std::shared_ptr<DeviceContext>& context = nullptr,
                                                                   const back_end::EdgeInformationOptions* information_options = nullptr) {
  std::vector<back_end::SubmapPairJob> jobs;
  for (const SubmapPair& p : ConsecutivePairs(submaps)) {
    back_end::SubmapPairJob j;
    j.source_submap_cloud = submaps[static_cast<size_t>(p.source)]->Cloud(context);                   // :417
    j.target_submap_cloud = submaps[static_cast<size_t>(p.target)]->Cloud(context);                   // :420
    j.source_first_frame_pose = submaps[static_cast<size_t>(p.source)]->FirstFramePose();
    j.target_first_frame_pose = submaps[static_cast<size_t>(p.target)]->FirstFramePose();
    jobs.push_back(j);
  }
  return back_end::SubmapPairMatchBatch(options, matcher, jobs, information_options);
}

}  // namespace builder
}  // namespace smhip

#endif  // SMHIP_SUBMAP_H_
