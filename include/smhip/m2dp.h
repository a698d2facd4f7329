// smhip/m2dp.h -- descriptor::M2dp of the reference (descriptor/m2dp.{h,cc}) over the device descriptor (smhip_m2dp_*,
// include/smhip.h).  Header-only, on top of smhip/filters.h (for the device context).
//
//   M2dp::M2dp                   m2dp.h:48-49   r = 0.1, max_distance = 100, t = 16, p = 4, q = 16
//   M2dp::setInputCloud          m2dp.cc:122-149  false for an empty cloud; preProcess, p*q views, the first singular pair of A
//   M2dp::getFinalDescriptor     m2dp.h:75
//   matchTwoM2dpDescriptors      m2dp.cc:151-169
// The descriptor is a std::vector<float> where the reference has an Eigen::VectorXf.  What the reference leaves open (pcl::PCA's
// projection, the sign of the singular pair) is defined in DESIGN.md section 6 ("M2DP").  setInputCloudResident is the device
// form: the descriptor of the cloud that lies in a handle's filter workspace (a filter chain's output, a built submap), without
// a download.
#ifndef SMHIP_M2DP_H_
#define SMHIP_M2DP_H_

#include <cstdio>
#include <memory>
#include <vector>

#include "smhip/filters.h"

namespace smhip {
namespace descriptor {

using DeviceContext = pre_processers::filter::DeviceContext;

class M2dp {
 public:
  using Descriptor = std::vector<float>;

  M2dp(double r = 0.1, double max_distance = 100., int32_t t = 16, int32_t p = 4, int32_t q = 16) {
    options_.r = r; options_.max_distance = max_distance; options_.t = t; options_.p = p; options_.q = q;
  }
  // the handle the descriptor is computed on (the process-wide default context when none is set)
  void SetDeviceContext(const std::shared_ptr<DeviceContext>& c) { context_ = c; }
  const smhip_m2dp_options& Options() const { return options_; }

  bool setInputCloud(const data::InnerCloudType::Ptr& source) {
    if (!source || source->points.empty()) {                                                  // m2dp.cc:123-126
      std::fprintf(stderr, "[ERROR] source is empty.\n");
      return false;
    }
    if (!context_) context_ = DeviceContext::Default();
    const int len = smhip_m2dp_length(&options_);
    if (len < 0) { std::fprintf(stderr, "[ERROR] the M2dp options are refused (r is too small, or beyond the device limits).\n"); return false; }
    Descriptor d(static_cast<size_t>(len));
    const smhip_status s = smhip_m2dp_f32(context_->handle(), &source->points[0].x, 5, static_cast<int>(source->points.size()), &options_, d.data(), len);
    return Done(context_->handle(), s, &d);
  }
  // the same for the cloud resident in `handle`'s filter workspace
  bool setInputCloudResident(smhip_handle handle) {
    const int len = smhip_m2dp_length(&options_);
    if (len < 0) { std::fprintf(stderr, "[ERROR] the M2dp options are refused (r is too small, or beyond the device limits).\n"); return false; }
    Descriptor d(static_cast<size_t>(len));
    return Done(handle, smhip_m2dp_from_filter_output(handle, &options_, d.data(), len), &d);
  }

  Descriptor getFinalDescriptor() const { return descriptor_; }

 private:
  bool Done(smhip_handle handle, smhip_status s, Descriptor* d) {
    if (s != SMHIP_OK) {
      std::fprintf(stderr, "[ERROR] smhip_m2dp: %s (%s)\n", smhip_status_string(s), smhip_last_error(handle));
      return false;
    }
    descriptor_.swap(*d);
    return true;
  }

  smhip_m2dp_options options_;
  std::shared_ptr<DeviceContext> context_;
  Descriptor descriptor_;
};

// the match score in (0, 1); -1 when the descriptors do not match in size or are shorter than 10
inline double matchTwoM2dpDescriptors(const M2dp::Descriptor& P, const M2dp::Descriptor& Q) {
  if (P.size() != Q.size() || P.size() < 10) {                                                // m2dp.cc:153-156
    std::fprintf(stderr, "[ERROR] The Descriptors do not match.\n");
    return -1.;
  }
  return smhip_m2dp_match(P.data(), Q.data(), static_cast<int>(P.size()));
}

}  // namespace descriptor
}  // namespace smhip

#endif  // SMHIP_M2DP_H_
