// smhip/front_end.h -- the front end's caller of the registrator boundary, restated over the GPU matchers.
// Header-only, on top of smhip/registrator.h and smhip/back_end.h (small matrix helpers).
//
//   MapBuilder::ScanMatchProcessing   /root/reference/builder/map_builder.cc:260-397
//       first cloud = first key frame (CalculateNormals for kFastIcp, :286); every later cloud is aligned against the
//       current KEY FRAME with guess = pose_target^-1 * extrapolated pose (:307-309), pose_source = pose_target *
//       align_result (:354); when the motion since the key frame passes the motion filter (translation_range /
//       angle_range, :370-383) the cloud becomes the next key frame (:384-392)
//   PoseExtrapolator (kSimpleCTRV)    /root/reference/builder/pose_extrapolator.cc:90-108, 177-197, 216-240, 296-317
//       constant velocity / turn rate from the oldest and newest pose of a short queue (lidar-only front end,
//       map_builder.cc:72-73)
//   MotionCompensation                /root/reference/builder/map_builder.cc:232-257, called at :320-328 and :336-352
//       the scan is de-skewed by the guess before SetInputSource and by the (averaged) result after Align; the second cloud is the
//       frame that goes on, and the next key frame when the motion filter fires.  "still in test" there, yet enabled by default
//       (map_builder.h:87-90) and in three of the four shipped configs.  Here: MotionCompensationOptions, DISABLED by default
//       (the KITTI config's setting); the host form below for any matcher, IcpFastHip's device form with device_target_prep
//   common::InterpolateTransform      /root/reference/common/math.h:199-211 (Eigen's Quaternion(Matrix3), slerp, toRotationMatrix)
//   common::AverageTransforms         /root/reference/common/math.cc:178-195
// Submap insertion and threading stay out: control plane.
#ifndef SMHIP_FRONT_END_H_
#define SMHIP_FRONT_END_H_

#include <cmath>
#include <deque>
#include <memory>
#include <utility>
#include <vector>

#include "smhip/back_end.h"
#include "smhip/registrator.h"

namespace smhip {
namespace front_end {

using registrator::Matrix4d;
using back_end::Multiply;
using back_end::NormalizeRotation;
using back_end::RigidInverse;
using InnerCloudPtr = data::InnerPointCloudData::Ptr;

// common/math.h:108-127 (x, y, z Euler angles of a rotation matrix)
inline void RotationMatrixToEulerAngles(const Matrix4d& R, double e[3]) {
  const double sy = std::sqrt(R(0, 0) * R(0, 0) + R(1, 0) * R(1, 0));
  if (!(sy < 1e-6)) { e[0] = std::atan2(R(2, 1), R(2, 2)); e[1] = std::atan2(-R(2, 0), sy); e[2] = std::atan2(R(1, 0), R(0, 0)); }
  else { e[0] = std::atan2(-R(1, 2), R(1, 1)); e[1] = std::atan2(-R(2, 0), sy); e[2] = 0; }
}
// common/math.h:130-138: Rz(e2) * Ry(e1) * Rx(e0)
inline Matrix4d EulerAnglesToRotation(const double e[3]) {
  const double cx = std::cos(e[0]), sx = std::sin(e[0]), cy = std::cos(e[1]), sy = std::sin(e[1]), cz = std::cos(e[2]), sz = std::sin(e[2]);
  Matrix4d R = Matrix4d::Identity();
  R(0, 0) = cz * cy; R(0, 1) = cz * sy * sx - sz * cx; R(0, 2) = cz * sy * cx + sz * sx;
  R(1, 0) = sz * cy; R(1, 1) = sz * sy * sx + cz * cx; R(1, 2) = sz * sy * cx - cz * sx;
  R(2, 0) = -sy;     R(2, 1) = cy * sx;                R(2, 2) = cy * cx;
  return R;
}

// Eigen::Quaternion<double>(Matrix3) of t's rotation block (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_op_impl):
// the trace branch, else the largest-diagonal branch, in which w may come out negative.  Not normalised.
struct Quaternion { double w = 1, x = 0, y = 0, z = 0; };
inline Quaternion QuaternionFromRotation(const Matrix4d& m) {
  Quaternion q;
  double v[3], t = m(0, 0) + m(1, 1) + m(2, 2);
  if (t > 0) {
    t = std::sqrt(t + 1.0); q.w = 0.5 * t; t = 0.5 / t;
    v[0] = (m(2, 1) - m(1, 2)) * t; v[1] = (m(0, 2) - m(2, 0)) * t; v[2] = (m(1, 0) - m(0, 1)) * t;
  } else {
    int i = 0; if (m(1, 1) > m(0, 0)) i = 1; if (m(2, 2) > m(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0); v[i] = 0.5 * t; t = 0.5 / t;
    q.w = (m(k, j) - m(j, k)) * t; v[j] = (m(j, i) + m(i, j)) * t; v[k] = (m(k, i) + m(i, k)) * t;
  }
  q.x = v[0]; q.y = v[1]; q.z = v[2];
  return q;
}
// q_a.slerp(t, q_b) of Eigen (Quaternion.h): what depends on the two quaternions alone is worked out once, At(t) is the rest.
// |d| >= 1 - DBL_EPSILON: the scales are 1 - t and t; otherwise sin((1 - t) theta) / sin(theta) and sin(t theta) / sin(theta) with
// theta = acos(|d|); the second scale is negated when d < 0; the result is NOT normalised.
struct Slerp {
  Quaternion a, b;
  double d = 1, theta = 0, sin_theta = 0;
  bool linear = true;
  Slerp(const Quaternion& qa, const Quaternion& qb) : a(qa), b(qb) {
    d = qa.x * qb.x + qa.y * qb.y + qa.z * qb.z + qa.w * qb.w;
    const double abs_d = std::fabs(d);
    linear = abs_d >= 1.0 - 2.220446049250313e-16;
    if (!linear) { theta = std::acos(abs_d); sin_theta = std::sin(theta); }
  }
  Quaternion At(double t) const {
    double scale0, scale1;
    if (linear) { scale0 = 1.0 - t; scale1 = t; }
    else { scale0 = std::sin((1.0 - t) * theta) / sin_theta; scale1 = std::sin(t * theta) / sin_theta; }
    if (d < 0) scale1 = -scale1;
    Quaternion q;
    q.x = scale0 * a.x + scale1 * b.x; q.y = scale0 * a.y + scale1 * b.y; q.z = scale0 * a.z + scale1 * b.z; q.w = scale0 * a.w + scale1 * b.w;
    return q;
  }
};
// Quaternion::toRotationMatrix of Eigen into R's rotation block
inline void QuaternionToRotation(const Quaternion& q, Matrix4d* R) {
  const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  (*R)(0, 0) = 1.0 - (tyy + tzz); (*R)(0, 1) = txy - twz; (*R)(0, 2) = txz + twy;
  (*R)(1, 0) = txy + twz; (*R)(1, 1) = 1.0 - (txx + tzz); (*R)(1, 2) = tyz - twx;
  (*R)(2, 0) = txz - twy; (*R)(2, 1) = tyz + twx; (*R)(2, 2) = 1.0 - (txx + tyy);
}
// common/math.h:199-211
inline Matrix4d InterpolateTransform(const Matrix4d& t1, const Matrix4d& t2, const float factor) {
  SMHIP_CHECK(factor >= 0. && factor <= 1., "CHECK(factor >= 0. && factor <= 1.)");       // :202
  Matrix4d out = Matrix4d::Identity();
  QuaternionToRotation(Slerp(QuaternionFromRotation(t1), QuaternionFromRotation(t2)).At(factor), &out);   // :204-206
  for (int i = 0; i < 3; ++i) out(i, 3) = t1(i, 3) + (t2(i, 3) - t1(i, 3)) * factor;      // :207-209
  return out;
}
// MotionCompensation, builder/map_builder.cc:232-257: row i moves by InterpolateTransform(I, delta, factor_i), the product in
// double, each coordinate cast to float, intensity and factor carried.  The two quaternions and the slerp's angle do not depend
// on the row and are worked out once; every row's numbers are those of the per-row call.  output may not be the input.
inline void MotionCompensation(const data::InnerCloudType& raw_cloud, const Matrix4d& delta_transform, data::InnerCloudType* const output_cloud) {
  SMHIP_CHECK(output_cloud != nullptr, "CHECK(output_cloud)");
  output_cloud->points.clear();
  output_cloud->stamp = raw_cloud.stamp;
  output_cloud->points.reserve(raw_cloud.points.size());
  const Matrix4d identity = Matrix4d::Identity();
  const Slerp slerp(QuaternionFromRotation(identity), QuaternionFromRotation(delta_transform));
  Matrix4d T = Matrix4d::Identity();
  for (const data::InnerPointType& point : raw_cloud.points) {
    SMHIP_CHECK(point.factor >= 0. && point.factor <= 1., "CHECK(factor >= 0. && factor <= 1.)");   // math.h:202
    const double f = point.factor;
    QuaternionToRotation(slerp.At(f), &T);
    const double x = point.x, y = point.y, z = point.z;
    data::InnerPointType new_point;
    new_point.x = static_cast<float>(((T(0, 0) * x + T(0, 1) * y) + T(0, 2) * z) + (0.0 + (delta_transform(0, 3) - 0.0) * f));   // :244-252
    new_point.y = static_cast<float>(((T(1, 0) * x + T(1, 1) * y) + T(1, 2) * z) + (0.0 + (delta_transform(1, 3) - 0.0) * f));
    new_point.z = static_cast<float>(((T(2, 0) * x + T(2, 1) * y) + T(2, 2) * z) + (0.0 + (delta_transform(2, 3) - 0.0) * f));
    new_point.intensity = point.intensity;
    new_point.factor = point.factor;
    output_cloud->points.push_back(new_point);
  }
}
// common/math.cc:178-195: the mean of the translations and of the x, y, z Euler angles
inline Matrix4d AverageTransforms(const std::vector<Matrix4d>& transforms) {
  SMHIP_CHECK(!transforms.empty(), "CHECK(!transforms.empty())");
  double angles[3] = {0, 0, 0}, translation[3] = {0, 0, 0};
  for (const Matrix4d& transform : transforms) {
    double e[3];
    RotationMatrixToEulerAngles(transform, e);
    for (int i = 0; i < 3; ++i) { translation[i] += transform(i, 3); angles[i] += e[i]; }
  }
  const double size = static_cast<double>(transforms.size());
  for (int i = 0; i < 3; ++i) { translation[i] /= size; angles[i] /= size; }
  Matrix4d result = EulerAnglesToRotation(angles);
  for (int i = 0; i < 3; ++i) result(i, 3) = translation[i];
  return result;
}

// PoseExtrapolator in Mode::kSimpleCTRV
class PoseExtrapolatorCTRV {
 public:
  explicit PoseExtrapolatorCTRV(double pose_queue_duration_s = 0.001) : duration_(pose_queue_duration_s) {}   // map_builder.cc:49
  bool Empty() const { return queue_.empty(); }
  double GetLastPoseTime() const { return queue_.empty() ? 0.0 : queue_.back().first; }
  void AddPose(double time, const Matrix4d& pose) {                         // pose_extrapolator.cc:90-108
    queue_.emplace_back(time, pose);
    if (queue_.size() == 1u) return;
    while (queue_.size() > 2 && queue_[1].first <= time - duration_) queue_.pop_front();
    UpdateVelocitiesFromPoses();
  }
  void InitRoughLinearVelocity(double vx, double vy, double vz) { linear_[0] = vx; linear_[1] = vy; linear_[2] = vz; }   // :210-214
  Matrix4d ExtrapolatePose(double time) const {                             // :177-197
    const Matrix4d& newest = queue_.back().second;
    const double dt = time - queue_.back().first;
    const double de[3] = {angular_[0] * dt, angular_[1] * dt, angular_[2] * dt};
    Matrix4d out = Multiply(RotationOnly(newest), EulerAnglesToRotation(de));   // newest rotation * delta (:185-188)
    for (int i = 0; i < 3; ++i) out(i, 3) = newest(i, 3) + dt * linear_[i];    // :183-184, :311-317
    return out;
  }

 private:
  static Matrix4d RotationOnly(const Matrix4d& t) { Matrix4d r = t; r(0, 3) = r(1, 3) = r(2, 3) = 0; return r; }
  void UpdateVelocitiesFromPoses() {                                         // :216-240
    if (queue_.size() < 2) return;
    const double delta = queue_.back().first - queue_.front().first;
    if (delta < duration_) return;
    const Matrix4d& a = queue_.front().second;
    const Matrix4d& b = queue_.back().second;
    for (int i = 0; i < 3; ++i) linear_[i] = (b(i, 3) - a(i, 3)) / delta;
    double e[3];
    RotationMatrixToEulerAngles(Multiply(RigidInverse(RotationOnly(a)), RotationOnly(b)), e);
    for (int i = 0; i < 3; ++i) angular_[i] = e[i] / delta;
  }
  double duration_;
  std::deque<std::pair<double, Matrix4d>> queue_;
  double linear_[3] = {0, 0, 0}, angular_[3] = {0, 0, 0};
};

// The guess for the next pair when T is the last pair's result, every scan is the next pair's target (a motion filter of 0) and the
// scans are equally spaced in time: [R_T, R_T^T t_T], normalised.  It is what PoseExtrapolatorCTRV + ProcessCloud form there: with
// poses P_k = P_{k-1} T the extrapolated pose is [R_k E(euler(R_T)), t_k + R_{k-1} t_T] (the linear velocity stays in the map
// frame, :170-177; E(euler(R)) = R below 90 degrees of pitch), and P_k^-1 times that is [R_T, R_k^T R_{k-1} t_T] (:261-262).
// smhip_shard --guess ctrv starts every pair from it (csrc/shard_driver.cc).
inline Matrix4d CtrvGuessFromLast(const Matrix4d& T) {
  Matrix4d g = Matrix4d::Identity();
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) g(i, j) = T(i, j);
    g(i, 3) = T(0, i) * T(0, 3) + T(1, i) * T(1, 3) + T(2, i) * T(2, 3);
  }
  NormalizeRotation(g);
  return g;
}

struct MotionFilter {                      // builder/map_builder.h:79-82
  float translation_range = 0.35f;
  float angle_range = 1.5f;                // degrees, sum of |Euler angles|
};

struct MotionCompensationOptions {         // builder/map_builder.h:87-90 (enable is true there; see the header comment)
  bool enable = false;
  bool use_average = true;
};

struct FrameResult {
  Matrix4d pose = Matrix4d::Identity();    // pose_source: the scan in the map frame
  Matrix4d guess = Matrix4d::Identity();
  Matrix4d align_result = Matrix4d::Identity();   // what the pose chain uses: with compensation and use_average, average_transform
  // motion compensation (identity when it is disabled, raw_result = align_result then)
  Matrix4d raw_result = Matrix4d::Identity();          // what the matcher's Align returned
  Matrix4d first_delta = Matrix4d::Identity();         // accumulative_transform^-1 * guess, :323-324
  Matrix4d second_delta = Matrix4d::Identity();        // accumulative_transform^-1 * average_transform, :349
  Matrix4d average_transform = Matrix4d::Identity();   // :337-344
  double score = 1.0;
  bool matched = false;                    // false for the first cloud (and while the extrapolator initialises)
  bool new_key_frame = false;
};

// MapBuilder::ScanMatchProcessing, one cloud per call
class ScanMatcherFrontEnd {
 public:
  // device_target_prep (IcpFastHip only): the key frame stays resident on the GPU.  Its normals are computed there
  // (SetInputTargetRaw / PromoteSourceToTarget) instead of the host CalculateNormals of map_builder.cc:286,389, the
  // target is not re-sent with every scan (the reference calls SetInputTarget per scan, :317), and a scan that becomes a
  // key frame is handed over from the source slot without a second upload.  false = the reference's call sequence.
  ScanMatcherFrontEnd(std::shared_ptr<registrator::Interface> scan_matcher, const MotionFilter& filter, bool use_extrapolator = true,
                      bool device_target_prep = false, const MotionCompensationOptions& motion_compensation = MotionCompensationOptions())
      : scan_matcher_(std::move(scan_matcher)), filter_(filter), use_extrapolator_(use_extrapolator), motion_compensation_(motion_compensation) {
    if (device_target_prep) device_icp_ = dynamic_cast<registrator::IcpFastHip*>(scan_matcher_.get());
  }
  bool DeviceTargetPrep() const { return device_icp_ != nullptr; }
  // Motion compensation (map_builder.cc:311-352).  Host form (any matcher without device_target_prep): the header's
  // MotionCompensation and the ordinary SetInputSource.  Device form (IcpFastHip with device_target_prep): the scan's rows go up
  // once (LoadScan), both passes are SetInputSourceCompensated on the device, and the second hands the rows back into the
  // caller's cloud.  Either way ProcessCloud REPLACES the points of the cloud it is given by the second pass's (SetInnerCloud, :351).
  void SetMotionCompensation(const MotionCompensationOptions& o) { motion_compensation_ = o; }
  const MotionCompensationOptions& MotionCompensationSettings() const { return motion_compensation_; }

  PoseExtrapolatorCTRV& Extrapolator() { return extrapolator_; }

  FrameResult ProcessCloud(const InnerCloudPtr& source_cloud, double source_time) {
    FrameResult out;
    if (!got_first_point_cloud_) {                                          // :280-293
      got_first_point_cloud_ = true;
      target_cloud_ = source_cloud;
      if (device_icp_) device_icp_->SetInputTargetRaw(target_cloud_);
      else if (scan_matcher_->GetType() == registrator::kFastIcp) target_cloud_->CalculateNormals();
      if (use_extrapolator_) extrapolator_.AddPose(source_time, Matrix4d::Identity());
      out.new_key_frame = true;
      return out;
    }
    if (use_extrapolator_ && source_time < extrapolator_.GetLastPoseTime()) {  // :296-300
      target_cloud_ = source_cloud;
      if (device_icp_) device_icp_->SetInputTargetRaw(target_cloud_);
      return out;
    }
    Matrix4d pose_source = pose_target_;
    if (use_extrapolator_) pose_source = extrapolator_.ExtrapolatePose(source_time);   // :302-305
    Matrix4d guess = Multiply(RigidInverse(pose_target_), pose_source);        // :307
    NormalizeRotation(guess);                                                  // :308
    Matrix4d align_result = Matrix4d::Identity();
    const bool compensate = motion_compensation_.enable;
    std::shared_ptr<data::InnerCloudType> inner_cloud_without_comp;            // :314
    if (compensate) { inner_cloud_without_comp = std::make_shared<data::InnerCloudType>(); inner_cloud_without_comp->points = source_cloud->GetInnerCloud(); }
    if (!device_icp_) scan_matcher_->SetInputTarget(target_cloud_);            // :317 (resident otherwise)
    if (compensate) {                                                          // :320-328
      out.first_delta = Multiply(RigidInverse(accumulative_transform_), guess);   // :323-324
      if (device_icp_) {
        device_icp_->LoadScan(std::shared_ptr<const std::vector<data::InnerPointType>>(inner_cloud_without_comp, &inner_cloud_without_comp->points));
        device_icp_->SetInputSourceCompensated(out.first_delta);
      } else {
        data::InnerCloudType compensated;
        MotionCompensation(*inner_cloud_without_comp, out.first_delta, &compensated);
        source_cloud->SetInnerCloud(compensated.points);                             // :327
        scan_matcher_->SetInputSource(source_cloud);                           // :329
      }
    } else {
      scan_matcher_->SetInputSource(source_cloud);                             // :329
    }
    scan_matcher_->Align(guess, align_result);                                 // :333
    out.raw_result = align_result;
    if (compensate) {                                                          // :336-352
      Matrix4d average_transform = align_result;
      if (motion_compensation_.use_average) {
        average_transform = AverageTransforms({align_result, guess});         // :339-342
        align_result = average_transform;                                      // :343
      }
      out.average_transform = average_transform;
      out.second_delta = Multiply(RigidInverse(accumulative_transform_), average_transform);   // :349
      if (device_icp_) {
        device_icp_->SetInputSourceCompensated(out.second_delta, source_cloud);
      } else {
        data::InnerCloudType compensated;
        MotionCompensation(*inner_cloud_without_comp, out.second_delta, &compensated);
        source_cloud->SetInnerCloud(compensated.points);                             // :351
      }
    }
    pose_source = Multiply(pose_target_, align_result);                        // :354
    accumulative_transform_ = align_result;                                    // :355
    if (use_extrapolator_) extrapolator_.AddPose(source_time, pose_source);    // :357
    out.pose = pose_source; out.guess = guess; out.align_result = align_result;
    out.score = scan_matcher_->GetFitnessScore(); out.matched = true;
    const double tx = accumulative_transform_(0, 3), ty = accumulative_transform_(1, 3), tz = accumulative_transform_(2, 3);
    const float accu_translation = static_cast<float>(std::sqrt(tx * tx + ty * ty + tz * tz));   // :370-371
    double e[3];
    RotationMatrixToEulerAngles(accumulative_transform_, e);
    const float accu_angles = static_cast<float>((std::fabs(e[0]) + std::fabs(e[1]) + std::fabs(e[2])) * (180. / M_PI));   // :374-377
    if (accu_translation >= filter_.translation_range || (filter_.angle_range > 1e-3 && accu_angles >= filter_.angle_range)) {   // :379-383
      accumulative_transform_ = Matrix4d::Identity();
      target_cloud_ = source_cloud;
      if (device_icp_) device_icp_->PromoteSourceToTarget();
      else if (scan_matcher_->GetType() == registrator::kFastIcp) target_cloud_->CalculateNormals();   // :389
      pose_target_ = pose_source;
      out.new_key_frame = true;
    }
    return out;
  }

 private:
  std::shared_ptr<registrator::Interface> scan_matcher_;
  MotionFilter filter_;
  bool use_extrapolator_;
  MotionCompensationOptions motion_compensation_;
  registrator::IcpFastHip* device_icp_ = nullptr;
  PoseExtrapolatorCTRV extrapolator_;
  bool got_first_point_cloud_ = false;
  InnerCloudPtr target_cloud_;
  Matrix4d pose_target_ = Matrix4d::Identity();
  Matrix4d accumulative_transform_ = Matrix4d::Identity();
};

}  // namespace front_end
}  // namespace smhip

#endif  // SMHIP_FRONT_END_H_
