// registrator::Interface::EnableInnerCompensation through the C++ mirror (include/smhip/registrator.h), the way
// builder/map_builder.cc drives a matcher: with the inner option "inner_compensation_mode" at 0 (default) the flag is refused, with
// 1 it selects the compensated iteration smhip.h defines.  Clouds come from KITTI-layout .bin files written by the pytest
// wrapper (tests/test_icp_compensation_gpu.py); the results go to stdout as JSON.
#define SMHIP_REGISTRATOR_THROW_ON_CHECK 1
#include <cmath>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "smhip/registrator.h"

using smhip::data::InnerPointCloudData;
using smhip::data::InnerPointType;
namespace reg = smhip::registrator;

static std::vector<InnerPointType> ReadKittiBin(const char* path) {
  std::ifstream f(path, std::ios::binary);
  std::vector<InnerPointType> pts;
  float v[4];
  while (f.read(reinterpret_cast<char*>(v), sizeof(v))) {
    InnerPointType p; p.x = v[0]; p.y = v[1]; p.z = v[2]; p.intensity = v[3]; p.factor = 0.f;
    pts.push_back(p);
  }
  for (size_t k = 0; k < pts.size(); ++k) pts[k].factor = static_cast<float>(k) / pts.size();
  return pts;
}

static void PrintMatrix(const char* name, const reg::Matrix4d& m) {
  std::printf("\"%s\": [", name);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) std::printf("%.17g%s", m(r, c), (r == 3 && c == 3) ? "" : ", ");
  std::printf("], ");
}

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s target.bin source.bin guess_tx\n", argv[0]); return 2; }
  InnerPointCloudData::Ptr target(new InnerPointCloudData(ReadKittiBin(argv[1])));
  InnerPointCloudData::Ptr source(new InnerPointCloudData(ReadKittiBin(argv[2])));
  target->CalculateNormals();
  reg::Matrix4d guess = reg::Matrix4d::Identity();
  guess(0, 3) = std::atof(argv[3]);
  const char* common = "<param name=\"max_iteration\"> 20 </param>";

  // mode 0 (default): refused, exactly as without the option; runs again once the flag is off
  reg::MatcherOptions opt0;
  opt0.type = reg::kFastIcp;
  opt0.registrator_options_node = std::string(common) + "<param name=\"inner_compensation_mode\"> 0 </param>";
  auto m0 = reg::CreateMatcher(opt0, true);
  if (!m0) return 3;
  m0->SetInputTarget(target);
  m0->SetInputSource(source);
  reg::Matrix4d rigid, r0;
  const bool rigid_ok = m0->Align(guess, rigid);
  m0->EnableInnerCompensation();
  bool refused = !m0->Align(guess, r0);
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) refused = refused && r0(r, c) == guess(r, c);
  m0->DisableInnerCompensation();
  bool off_runs = m0->Align(guess, r0);
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) off_runs = off_runs && r0(r, c) == rigid(r, c);

  // mode 1: the flag selects the compensated iteration; without the flag the same matcher aligns rigidly, bit for bit
  reg::MatcherOptions opt1 = opt0;
  opt1.registrator_options_node = std::string(common) + "<param name=\"inner_compensation_mode\"> 1 </param>";
  auto m1 = reg::CreateMatcher(opt1, true);
  if (!m1) return 3;
  m1->SetInputTarget(target);
  m1->SetInputSource(source);
  reg::Matrix4d comp, r1;
  m1->EnableInnerCompensation();
  const bool comp_ok = m1->Align(guess, comp);
  const double comp_score = m1->GetFitnessScore();
  m1->DisableInnerCompensation();
  bool rigid_again = m1->Align(guess, r1);
  for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) rigid_again = rigid_again && r1(r, c) == rigid(r, c);

  std::printf("{");
  PrintMatrix("rigid", rigid);
  PrintMatrix("compensated", comp);
  std::printf("\"rigid_ok\": %s, \"refused_in_mode_0\": %s, \"mode_0_off_runs\": %s, \"compensated_ok\": %s, \"compensated_score\": %.17g, "
              "\"mode_1_off_is_rigid\": %s, \"target_points\": %d}\n",
              rigid_ok ? "true" : "false", refused ? "true" : "false", off_runs ? "true" : "false", comp_ok ? "true" : "false", comp_score,
              rigid_again ? "true" : "false", target->GetEigenCloud()->size());
  return 0;
}
