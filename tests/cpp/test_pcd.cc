// include/smhip/pcd.h on its own (no HIP, no PCL): writes the rows of a raw float32 file as a PCD file, for tests/test_pcd_io.py
// to compare with the Python writer byte for byte.  Usage: test_pcd ROWS.bin N rgb(0|1) OUT.pcd -- exit 0 when a file was written,
// 1 when not (an empty cloud).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "smhip/pcd.h"

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: test_pcd ROWS.bin N rgb OUT.pcd\n"); return 2; }
  const size_t n = std::strtoul(argv[2], nullptr, 10);
  std::vector<float> rows(4 * n + 4);
  if (n > 0) {
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(rows.data(), 16, n, f) != n) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::fclose(f);
  }
  return smhip::pcd::SaveBinary(argv[4], n > 0 ? rows.data() : nullptr, n, std::atoi(argv[3]) != 0) ? 0 : 1;
}
