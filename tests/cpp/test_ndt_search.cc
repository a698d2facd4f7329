// registrator::NdtHip's inner option "search_method" set the way builder/map_builder.cc sets every matcher option: through the
// option registry, from the XML node of MatcherOptions.  usage: test_ndt_search target.bin source.bin guess_tx search_method
// Clouds are KITTI-layout .bin files (float32 x, y, z, intensity) written by the pytest wrapper; the result goes to stdout as JSON:
// one Align under the option, and the same pair twice through AlignBatch.
#define SMHIP_REGISTRATOR_THROW_ON_CHECK 1
#include <cstdio>
#include <cstdlib>
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
  return pts;
}

static void PrintMatrix(const char* name, const reg::Matrix4d& m) {
  std::printf("\"%s\": [", name);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) std::printf("%.17g%s", m(r, c), (r == 3 && c == 3) ? "" : ", ");
  std::printf("]");
}

int main(int argc, char** argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: %s target.bin source.bin guess_tx search_method\n", argv[0]); return 2; }
  reg::MatcherOptions opt;
  opt.type = reg::kNdt;
  opt.registrator_options_node = std::string("<param name=\"search_method\"> ") + argv[4] + " </param>";
  auto matcher = reg::CreateMatcher(opt);
  auto* ndt = dynamic_cast<reg::NdtHip*>(matcher.get());
  if (!ndt) return 3;
  InnerPointCloudData::Ptr target(new InnerPointCloudData(ReadKittiBin(argv[1])));
  InnerPointCloudData::Ptr source(new InnerPointCloudData(ReadKittiBin(argv[2])));
  reg::Matrix4d guess = reg::Matrix4d::Identity(), result = reg::Matrix4d::Identity();
  guess(0, 3) = std::atof(argv[3]);
  ndt->SetInputTarget(target);
  ndt->SetInputSource(source);
  const bool ok = ndt->Align(guess, result);
  const smhip_ndt_stats st = ndt->LastStats();
  std::vector<reg::Matrix4d> results;
  std::vector<double> scores;
  std::vector<smhip_ndt_stats> bst;
  const bool batch_ok = ndt->AlignBatch({source, source}, {target, target}, {guess, guess}, &results, &scores, &bst);
  bool batch_same = batch_ok && results.size() == 2 && bst.size() == 2;
  for (int k = 0; batch_same && k < 2; ++k) {
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) batch_same = batch_same && results[k](r, c) == result(r, c);
    batch_same = batch_same && bst[k].pairs_last == st.pairs_last && bst[k].iterations == st.iterations && scores[k] == ndt->GetFitnessScore();
  }
  std::printf("{\"ok\": %s, \"batch_same\": %s, \"score\": %.17g, \"iterations\": %d, \"derivative_calls\": %d, \"pairs_last\": %.17g, ",
              ok ? "true" : "false", batch_same ? "true" : "false", ndt->GetFitnessScore(), st.iterations, st.derivative_calls, st.pairs_last);
  PrintMatrix("result", result);
  std::printf("}\n");
  return 0;
}
