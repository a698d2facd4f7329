// smhip/align_information.h -- smhip_icp_information (include/smhip.h) as a C++ value: what a registrator's GetInformation hands out.
// Header-only, host-only.  The back end turns it into a pose-graph edge (smhip/edge_information.h); the matcher layer knows nothing of that.
#ifndef SMHIP_ALIGN_INFORMATION_H_
#define SMHIP_ALIGN_INFORMATION_H_

#include <array>
#include <cstddef>

#include "../smhip.h"

namespace smhip {
namespace registrator {

// H row-major, symmetric, in the tangent of the pose graph's BETWEEN residual (rotation first)
struct AlignInformation {
  std::array<double, 36> H{};
  double sum_r2 = 0.0;
  double limit_d2 = 0.0;
  int kept = 0;
  int n_finite = 0;
};

inline AlignInformation FromAbi(const smhip_icp_information& in) {
  AlignInformation out;
  for (int k = 0; k < 36; ++k) out.H[static_cast<size_t>(k)] = in.H[k];
  out.sum_r2 = in.sum_r2; out.limit_d2 = in.limit_d2; out.kept = in.kept; out.n_finite = in.n_finite;
  return out;
}

}  // namespace registrator
}  // namespace smhip

#endif  // SMHIP_ALIGN_INFORMATION_H_
