// Host test of the grid-build choice in staticmapping_amd/csrc/icp_plan.h (plan::sorted_grid_build): which launches build the ICP
// search grid by one in-LDS sort per pair (grid_sort_build.hip) and which keep the mark / rank / count / place kernels.
// Built with g++ alone (tests/test_grid_plan_cpp.py); no device, no HIP library.
#include <cstdio>

#include "icp_plan.h"

using namespace smhip;
using namespace smhip::plan;

namespace {
long g_checks = 0, g_failures = 0;
#define CHECK(cond)                                                                              \
  do {                                                                                           \
    ++g_checks;                                                                                  \
    if (!(cond)) { ++g_failures; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)
}  // namespace

int main() {
  const int grid = SMHIP_NN_GRID;
  // the ICP batch's targets: GRID, cells sorted, no row bitmap
  CHECK(sorted_grid_build(1, grid, 1, 0, 512, 21700));
  CHECK(sorted_grid_build(1, grid, 1, 0, 256, 1));
  // the size limit: one workgroup of 1 024 threads x 32 points, the shadow word's 15-bit match
  CHECK(kSortBuildMaxTarget == 32768 && kSortBuildMaxTarget == kShadowMaxTarget + 1);
  CHECK(sorted_grid_build(1, grid, 1, 0, 64, 32768));
  CHECK(!sorted_grid_build(1, grid, 1, 0, 64, 32769));
  CHECK(!sorted_grid_build(1, grid, 1, 0, 1, 500000));      // the NDT / GICP targets
  // everything that is not that grid keeps the kernels it had
  CHECK(!sorted_grid_build(1, grid, 0, 0, 64, 5000));       // sort_cells = 0
  CHECK(!sorted_grid_build(1, grid, 1, 1, 64, 5000));       // the ring searches' row bitmap
  CHECK(!sorted_grid_build(1, SMHIP_NN_NABO, 1, 0, 64, 5000));
  CHECK(!sorted_grid_build(1, SMHIP_NN_BRUTE, 1, 0, 64, 5000));
  // SMHIP_GRID_BUILD=0
  CHECK(!sorted_grid_build(0, grid, 1, 0, 512, 21700));
  CHECK(!sorted_grid_build(0, grid, 1, 0, 1, 1));
  // the pair-count threshold the measurement set
  CHECK(kSortBuildMinPairs >= 1);
  CHECK(sorted_grid_build(1, grid, 1, 0, kSortBuildMinPairs, 21700));
  CHECK(!sorted_grid_build(1, grid, 1, 0, kSortBuildMinPairs - 1, 21700));
  for (int np = 1; np <= 1024; ++np) CHECK(sorted_grid_build(1, grid, 1, 0, np, 21700) == (np >= kSortBuildMinPairs));
  std::printf("%ld checks, %ld failed\n", g_checks, g_failures);
  if (g_failures) return 1;
  std::printf("all checks passed\n");
  return 0;
}
