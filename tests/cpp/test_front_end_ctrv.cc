// front_end::CtrvGuessFromLast against the guess ScanMatcherFrontEnd forms (PoseExtrapolatorCTRV + ProcessCloud) when it is fed the same
// poses: use_extrapolator, a stub matcher that returns a prescribed result, a motion filter of 0 (every scan becomes the next key
// frame), scans equally spaced in time.  No device work: the stub is not IcpFastHip and its type asks for no normals.
// Prints one JSON line: the number of guesses compared, the largest entry-wise difference, and -- so that the comparison cannot pass on
// a formula that ignores the motion -- the largest difference between the guess and the last result itself.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "smhip/front_end.h"

using smhip::registrator::Matrix4d;
namespace fe = smhip::front_end;

namespace {

struct StubMatcher : smhip::registrator::Interface {
  Matrix4d next = Matrix4d::Identity();
  bool Align(const Matrix4d&, Matrix4d& result) override { result = next; this->final_score_ = 1.0; return true; }
};

uint64_t g_state = 0x9e3779b97f4a7c15ull;
double U01() {                      // splitmix64
  uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return static_cast<double>(z >> 11) * (1.0 / 9007199254740992.0);
}

// rotation by up to max_angle about a random axis, translation of up to max_t metres in a random direction
Matrix4d RandomMotion(double max_angle, double max_t) {
  double ax[3], n = 0;
  do { n = 0; for (double& v : ax) { v = 2 * U01() - 1; n += v * v; } } while (n < 1e-4 || n > 1);
  n = std::sqrt(n);
  for (double& v : ax) v /= n;
  const double ang = max_angle * (2 * U01() - 1), c = std::cos(ang), s = std::sin(ang), v = 1 - c;
  Matrix4d T = Matrix4d::Identity();
  T(0, 0) = c + v * ax[0] * ax[0]; T(0, 1) = v * ax[0] * ax[1] - s * ax[2]; T(0, 2) = v * ax[0] * ax[2] + s * ax[1];
  T(1, 0) = v * ax[0] * ax[1] + s * ax[2]; T(1, 1) = c + v * ax[1] * ax[1]; T(1, 2) = v * ax[1] * ax[2] - s * ax[0];
  T(2, 0) = v * ax[0] * ax[2] - s * ax[1]; T(2, 1) = v * ax[1] * ax[2] + s * ax[0]; T(2, 2) = c + v * ax[2] * ax[2];
  double d[3], m = 0;
  do { m = 0; for (double& e : d) { e = 2 * U01() - 1; m += e * e; } } while (m < 1e-4 || m > 1);
  const double len = max_t * U01() / std::sqrt(m);
  for (int i = 0; i < 3; ++i) T(i, 3) = d[i] * len;
  return T;
}

}  // namespace

int main() {
  const int kChains = 100, kLength = 4;          // 400 guesses, each behind a different pose history
  const double kStep = 0.125;                     // seconds between scans (exact in binary: equal spacing is exact)
  const std::vector<smhip::data::InnerPointType> one_point(1);
  int cases = 0;
  double worst = 0, worst_vs_result = 0;
  for (int chain = 0; chain < kChains; ++chain) {
    auto stub = std::make_shared<StubMatcher>();
    fe::ScanMatcherFrontEnd front(stub, fe::MotionFilter{0.f, 0.f}, /*use_extrapolator=*/true);
    double t = 0;
    front.ProcessCloud(std::make_shared<smhip::data::InnerPointCloudData>(one_point), t);
    Matrix4d last = Matrix4d::Identity();
    for (int k = 0; k <= kLength; ++k) {
      t += kStep;
      stub->next = RandomMotion(20.0 * M_PI / 180.0, 3.0);
      const fe::FrameResult out = front.ProcessCloud(std::make_shared<smhip::data::InnerPointCloudData>(one_point), t);
      if (!out.matched || !out.new_key_frame) { std::printf("{\"error\": \"scan %d of chain %d was not matched and promoted\"}\n", k, chain); return 1; }
      if (k > 0) {                                // (the first pair has no history: the extrapolator holds one pose)
        const Matrix4d want = fe::CtrvGuessFromLast(last);
        for (int i = 0; i < 16; ++i) {
          worst = std::max(worst, std::fabs(out.guess.m[i] - want.m[i]));
          worst_vs_result = std::max(worst_vs_result, std::fabs(out.guess.m[i] - last.m[i]));
        }
        ++cases;
      }
      last = out.align_result;
    }
  }
  std::printf("{\"cases\": %d, \"worst\": %.3e, \"worst_vs_result\": %.3e}\n", cases, worst, worst_vs_result);
  return 0;
}
