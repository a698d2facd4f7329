// smhip_ndt_gicp.hip -- the NDT / NdtWithGicp translation unit of libsmhip.so: registrators::Ndt and registrators::NdtWithGicp,
// kernels and hosts, as four fragments in this order.  They are one unit because the GICP host drives the NDT engine directly
// (NdtWithGicp::Align is NDT first, then GICP from its pose: ndt_ensure, ndt_align_slots, fitness_scores) and gicp_kernels.hip
// uses ndt_kernels.hip's jacobi_eig3.  The handle and the ICP unit's functions it calls (grid build, FindClosests) come from
// smhip_context.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "smhip_context.h"

using namespace smhip_host;
using plan::ceil_div;

// ndt_kernels.hip uses the wave reductions and the block scan of kd_median_tree.h without including it.  The file is kept
// byte for byte (profiles/traffic_ndt_derivatives_ctl.json is dated with its hash), so what it needs is included here.
#include "smhip_device.h"
#include "kd_median_tree.h"
#include "ndt_kernels.hip"
#include "smhip_ndt_api.hip"
#include "gicp_kernels.hip"
#include "smhip_gicp_api.hip"
