// test_ndt_ctl.cc -- runs the serial end of Ndt (staticmapping_amd/csrc/ndt_ctl_math.h: ndt_solve6, svd_solve6 and the Newton /
// More-Thuente state machine) on the host.  tests/test_ndt_ctl_cpp.py talks to it over its standard input and output, a line at a
// time; g++ alone (-D__HIP_PLATFORM_AMD__), no device; built a second time with -fsanitize=address,undefined.
//
//   solve H[36] b[6]                              -> solve x[6] | svd x[6]      (ndt_solve6, and svd_solve6 on the same system)
//   mt a_l f_l g_l a_u f_u g_u a_t f_t g_t        -> mt converged trial_value a_l f_l g_l a_u f_u g_u  (trial_value_mt, then
//                                                    update_interval_mt on the same nine numbers)
//   run step_size trans_eps max_iterations p0[6]  -> the machine's requests, one at a time:
//        req phase compute_hessian eval_p[6]         answered by the caller with   val score g[6] H[36]
//      and at the end
//        end it deriv_calls phase p[6] sc g[6] H[36]
//   quit
// The objective lives with the caller: both this machine and the reference restatement are answered by the same function.
// Numbers travel as C99 hex floats: every bit arrives.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ndt_ctl_math.h"

static bool read_doubles(double* v, int n) {
  char tok[64];
  for (int i = 0; i < n; ++i) {
    if (scanf("%63s", tok) != 1) return false;
    v[i] = strtod(tok, nullptr);
  }
  return true;
}
static void put(const double* v, int n) {
  for (int i = 0; i < n; ++i) printf(" %a", v[i]);
}

int main() {
  char kind[32];
  long cases = 0;
  while (scanf("%31s", kind) == 1) {
    const std::string k = kind;
    if (k == "quit") break;
    if (k == "solve") {
      double H[36], b[6], x[6], xs[6];
      if (!read_doubles(H, 36) || !read_doubles(b, 6)) return 3;
      for (int i = 0; i < 6; ++i) x[i] = xs[i] = -777.0;               // a branch that leaves an entry unwritten shows
      smhip::ndt_solve6(H, b, x);
      smhip::svd_solve6(H, b, xs);
      printf("solve"); put(x, 6); printf(" | svd"); put(xs, 6); printf("\n");
    } else if (k == "mt") {
      double v[9];                                                       // a_l f_l g_l a_u f_u g_u a_t f_t g_t
      if (!read_doubles(v, 9)) return 3;
      const double a = smhip::trial_value_mt(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]);
      const bool conv = smhip::update_interval_mt(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]);
      printf("mt %d", conv ? 1 : 0); put(&a, 1); put(v, 6); printf("\n");
    } else if (k == "run") {
      double opt[3], p0[6];
      if (!read_doubles(opt, 3) || !read_doubles(p0, 6)) return 3;
      smhip::NdtCtlOpts o;
      memset(&o, 0, sizeof(o));
      o.step_size = opt[0]; o.trans_eps = opt[1]; o.max_iterations = (int32_t)opt[2];
      // a job's state before its first evaluation, as ndt_ctl_start leaves it
      static smhip::NdtCtl j;
      memset(&j, 0, sizeof(j));
      for (int i = 0; i < 6; ++i) j.p[i] = j.eval_p[i] = p0[i];
      j.phase = smhip::kNdtInit;
      j.pose.compute_hessian = 1;
      long rounds = 0;
      while (j.phase != smhip::kNdtDone) {
        if (++rounds > 100000) { fprintf(stderr, "the machine does not end\n"); return 4; }
        printf("req %d %d", (int)j.phase, (int)j.pose.compute_hessian); put(j.eval_p, 6); printf("\n");
        fflush(stdout);
        char tok[32];
        double out[44];
        if (scanf("%31s", tok) != 1 || std::string(tok) != "val" || !read_doubles(out, 43)) return 3;
        out[43] = (double)rounds;                                      // the pair count column: carried, never decided on
        smhip::ndt_ctl_result(j, out, o);
      }
      printf("end %d %d %d", (int)j.it, (int)j.deriv_calls, (int)j.phase); put(j.p, 6); put(&j.sc, 1); put(j.g, 6); put(j.H, 36); printf("\n");
    } else {
      fprintf(stderr, "unknown command %s\n", kind);
      return 3;
    }
    fflush(stdout);
    ++cases;
  }
  printf("done %ld\n", cases);
  return 0;
}
