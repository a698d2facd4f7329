// sweep_motion.h -- the sensor's motion during every frame's sweep, from the trajectory alone: what the map builder de-skews a frame
// by once the poses are final ("Motion compensation after optimisation").  Host only: the standard library,
// no device, no Eigen.
//
// A frame's pose is the sensor pose at the START of its sweep (ScanMatcherFrontEnd::ProcessCloud aligns and stores the cloud
// de-skewed into that frame), so the motion during sweep k is the step to the next frame's pose:
//     delta_k     = RigidInverse(P_k) * P_{k+1}      for k < n - 1
//     delta_{n-1} = delta_{n-2}                      the last frame has no successor: it repeats its predecessor's motion
//     n == 1:       the identity
// RigidInverse is (R^T, -R^T t), as everywhere in front_end.h.  The poses are the whole run's, in file order: which frames a map
// inserts (every K-th, say) does not change which two poses define a frame's motion.
#pragma once

#include <array>
#include <cstddef>
#include <vector>

namespace smhip {

using Pose = std::array<double, 16>;                                      // column-major 4x4: m[4 * c + r]

namespace sweep_motion_detail {

inline Pose Identity() { return Pose{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}; }

inline Pose RigidInverse(const Pose& t) {
  Pose r = Identity();
  for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r[4 * j + i] = t[4 * i + j];
  for (int i = 0; i < 3; ++i) r[12 + i] = -(r[i] * t[12] + r[4 + i] * t[13] + r[8 + i] * t[14]);
  return r;
}

inline Pose Multiply(const Pose& a, const Pose& b) {
  Pose out{};
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) { double s = 0; for (int k = 0; k < 4; ++k) s += a[4 * k + r] * b[4 * c + k]; out[4 * c + r] = s; }
  return out;
}

}  // namespace sweep_motion_detail

inline std::vector<Pose> SweepMotions(const std::vector<Pose>& poses) {
  namespace d = sweep_motion_detail;
  const std::size_t n = poses.size();
  std::vector<Pose> motions(n, d::Identity());
  for (std::size_t k = 0; k + 1 < n; ++k) motions[k] = d::Multiply(d::RigidInverse(poses[k]), poses[k + 1]);
  if (n >= 2) motions[n - 1] = motions[n - 2];
  return motions;
}

}  // namespace smhip
