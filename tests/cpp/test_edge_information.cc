// test_edge_information.cc -- smhip/edge_information.h driven from tests/test_edge_information_cpp.py: no device, no library.
//   test_edge_information IN OUT
// IN: int32 count, then per case 48 doubles: H[36] row-major, sum_r2, kept, min_residual_sigma, information_scale, max_inflation,
// a flag (0: the default floor; 1: the six sigmas that follow -- the case then has 54 doubles), padding to 48.
// OUT per case 91 doubles: L[36], strength[6], weakest[6], residual_sigma, then JacobiEigen6 of H itself: w[6], Q[36].
// Every case is computed twice; bits that differ between the two end the program with status 2.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "smhip/edge_information.h"

using namespace smhip::back_end;

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: test_edge_information IN OUT\n"); return 1; }
  std::FILE* in = std::fopen(argv[1], "rb");
  if (!in) { std::perror(argv[1]); return 1; }
  int32_t count = 0;
  if (std::fread(&count, sizeof(count), 1, in) != 1 || count < 0) return 1;
  std::vector<double> out;
  for (int k = 0; k < count; ++k) {
    double row[48];
    if (std::fread(row, sizeof(double), 48, in) != 48) return 1;
    AlignInformation info;
    for (int i = 0; i < 36; ++i) info.H[i] = row[i];
    info.sum_r2 = row[36];
    info.kept = static_cast<int>(row[37]);
    EdgeInformationOptions options;
    options.min_residual_sigma = row[38];
    options.information_scale = row[39];
    options.max_inflation = row[40];
    if (row[41] != 0.0) {
      double floor[6];
      if (std::fread(floor, sizeof(double), 6, in) != 6) return 1;
      for (int i = 0; i < 6; ++i) options.floor[i] = floor[i];
    }
    double got[2][91];
    for (int pass = 0; pass < 2; ++pass) {
      const EdgeInformation e = MakeEdgeInformation(info, options);
      if (e.kept != info.kept) return 3;
      double* g = got[pass];
      for (int i = 0; i < 36; ++i) g[i] = e.sqrt_information[i];
      for (int i = 0; i < 6; ++i) { g[36 + i] = e.strength[i]; g[42 + i] = e.weakest[i]; }
      g[48] = e.residual_sigma;
      std::array<double, 6> w;
      std::array<double, 36> Q;
      JacobiEigen6(info.H, &w, &Q);
      for (int i = 0; i < 6; ++i) g[49 + i] = w[i];
      for (int i = 0; i < 36; ++i) g[55 + i] = Q[i];
    }
    if (std::memcmp(got[0], got[1], sizeof(got[0])) != 0) { std::fprintf(stderr, "case %d: two calls differ\n", k); return 2; }
    out.insert(out.end(), got[0], got[0] + 91);
  }
  std::fclose(in);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 1; }
  std::fwrite(out.data(), sizeof(double), out.size(), o);
  std::fclose(o);
  std::printf("%d cases\n", count);
  return 0;
}
