// include/smhip/sweep_motion.h, host only, no library:
//   test_sweep_motion <poses_in> <poses_out>
// <poses_in>: a pose per line at full precision (12 numbers, the row-major top 3 x 4).  The program writes them to <poses_out> as the
// pose writer does (8 significant digits), reads that file back with ReadPoses and prints smhip::SweepMotions of what it read: one
// line per frame, the 16 numbers of the column-major 4 x 4 with 17 significant digits.  tests/test_sweep_motion_cpp.py compares them
// with the numpy restatement (tests/map_compensation_ref.py).  It also checks on its own that the last motion repeats its
// predecessor, that one pose gives the identity and none gives nothing.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/smhip/sweep_motion.h"
#include "../../staticmapping_amd/csrc/shard_poses.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: test_sweep_motion <poses_in> <poses_out>\n"); return 2; }
  std::vector<shard::Pose> exact;
  if (!shard::ReadPoses(argv[1], &exact)) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  {
    std::ofstream out(argv[2]);
    out.precision(8);                                                     // the pose writer's
    for (const shard::Pose& p : exact) shard::WritePoseLine(out, p.data());
  }
  std::vector<shard::Pose> poses;                                         // (shard::Pose and smhip::Pose are one type)
  EXPECT(shard::ReadPoses(argv[2], &poses) && poses.size() == exact.size());
  const std::vector<smhip::Pose> motions = smhip::SweepMotions(poses);
  EXPECT(motions.size() == poses.size());
  const size_t n = motions.size();
  if (n >= 2) EXPECT(std::memcmp(motions[n - 1].data(), motions[n - 2].data(), sizeof(double) * 16) == 0);
  const smhip::Pose identity{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (n == 1) EXPECT(motions[0] == identity);
  EXPECT(smhip::SweepMotions({}).empty());
  if (!poses.empty()) {
    const std::vector<smhip::Pose> one = smhip::SweepMotions({poses[0]});
    EXPECT(one.size() == 1 && one[0] == identity);
  }
  for (const smhip::Pose& m : motions) {
    for (int q = 0; q < 16; ++q) std::printf("%.17g%s", m[q], q == 15 ? "\n" : " ");
  }
  if (failures == 0) std::printf("all checks passed\n");
  return failures == 0 ? 0 : 1;
}
