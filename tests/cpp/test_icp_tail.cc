// test_icp_tail.cc -- runs the arithmetic of IcpFast's iteration tail (staticmapping_amd/csrc/icp_tail_math.h) on the host, case by
// case: tests/test_icp_tail_cpp.py writes the cases, this program answers them line for line, and the test compares the answers
// with a multi-precision reference.  g++ alone (-D__HIP_PLATFORM_AMD__), no device; built a second time with
// -fsanitize=address,undefined.
//
//   solve  A[36] b[6]          -> branch x[6]
//   quat   R[9]                -> q[4]
//   qdist  a[4] c[4]           -> d
//   aa     x[6]                -> dT[12]   (rows of the 3x4)
//   pot    Mnew[12] Mold[12]   -> step_a step_b
//   ring   early n T[12] * n   -> n lines "converged n_hist", then the ring: n_hist rows of quat[4] trans[3]
// Numbers travel as C99 hex floats: every bit arrives.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "icp_tail_math.h"

static bool read_doubles(FILE* f, double* v, int n) {
  char tok[64];
  for (int i = 0; i < n; ++i) {
    if (fscanf(f, "%63s", tok) != 1) return false;
    v[i] = strtod(tok, nullptr);
  }
  return true;
}
static void put(const double* v, int n) {
  for (int i = 0; i < n; ++i) printf(" %a", v[i]);
}
static void pose_from_rows(const double* r12, double* T) {
  for (int i = 0; i < 12; ++i) T[i] = r12[i];
  T[12] = 0; T[13] = 0; T[14] = 0; T[15] = 1;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  char kind[32];
  long cases = 0;
  while (fscanf(f, "%31s", kind) == 1) {
    const std::string k = kind;
    if (k == "solve") {
      double A[36], b[6], x[6];
      if (!read_doubles(f, A, 36) || !read_doubles(f, b, 6)) return 3;
      for (int i = 0; i < 6; ++i) x[i] = -777.0;                     // a branch that leaves an entry unwritten shows
      const int br = smhip::solve6(A, b, x);
      printf("solve %d", br); put(x, 6); printf("\n");
    } else if (k == "quat") {
      double R[9], T[16] = {0}, q[4];
      if (!read_doubles(f, R, 9)) return 3;
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) T[4 * i + j] = R[3 * i + j];
      smhip::quat_from_rot(T, q);
      printf("quat"); put(q, 4); printf("\n");
    } else if (k == "qdist") {
      double a[4], c[4];
      if (!read_doubles(f, a, 4) || !read_doubles(f, c, 4)) return 3;
      const double d = smhip::quat_angular_distance(a, c);
      printf("qdist"); put(&d, 1); printf("\n");
    } else if (k == "aa") {
      double x[6];
      if (!read_doubles(f, x, 6)) return 3;
      double dT[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
      smhip::angle_axis_step(x, dT);
      printf("aa"); put(dT, 12); printf("\n");
    } else if (k == "pot") {
      double a[12], b[12], Mn[16], Mo[16], sa, sb;
      if (!read_doubles(f, a, 12) || !read_doubles(f, b, 12)) return 3;
      pose_from_rows(a, Mn); pose_from_rows(b, Mo);
      smhip::motion_potential_step(Mn, Mo, &sa, &sb);
      printf("pot"); put(&sa, 1); put(&sb, 1); printf("\n");
    } else if (k == "ring") {
      int early = 0, n = 0;
      if (fscanf(f, "%d %d", &early, &n) != 2 || n < 0 || n > 64) return 3;
      double quat[5][4], trans[5][3];
      memset(quat, 0, sizeof(quat)); memset(trans, 0, sizeof(trans));
      quat[0][0] = 1.0;                                               // the state an Align starts from: the identity, one entry
      int32_t nh = 1;
      printf("ring %d\n", n);
      for (int s = 0; s < n; ++s) {
        double r[12], T[16];
        if (!read_doubles(f, r, 12)) return 3;
        pose_from_rows(r, T);
        const bool conv = smhip::history_push_converged(quat, trans, &nh, T, early != 0);
        printf("push %d %d\n", conv ? 1 : 0, (int)nh);
      }
      for (int h = 0; h < nh; ++h) { printf("entry"); put(quat[h], 4); put(trans[h], 3); printf("\n"); }
    } else {
      fprintf(stderr, "unknown case kind %s\n", kind);
      return 3;
    }
    ++cases;
  }
  fclose(f);
  printf("done %ld\n", cases);
  return 0;
}
