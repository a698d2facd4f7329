// include/smhip/map_package.h without a device: PlanMapPackage, the description file and the failure mode of a package written
// into a missing directory.  tests/test_map_package_cpp.py feeds the cases and compares with tests/map_package_ref.py.
//
//   test_map_package plan IN         IN: doubles n, border_offset, piece_width, then n x 3 translations.  Prints "refused <why>", or
//                                    "steps X Y" and per piece "piece x y cx cy minx miny maxx maxy k m0 .. mk-1", doubles as %.17g
//   test_map_package xml IN DIR      the plan of IN written to DIR/map_package.xml twice (must be the same bytes) and into
//                                    DIR/missing/ (must fail and leave nothing)
//   test_map_package save DIR        SaveTrajectoriesAsMapPackage into DIR/missing/ : false before any device work, nothing written;
//                                    a refused plan: false, nothing written
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "smhip/map_package.h"

namespace {

#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } } while (0)

bool ReadCase(const char* path, std::vector<std::array<double, 3>>* t, smhip::MapPackageOptions* o) {
  std::ifstream f(path, std::ios::binary);
  double head[3];
  if (!f.read(reinterpret_cast<char*>(head), sizeof(head))) return false;
  o->border_offset = head[1]; o->piece_width = head[2];
  t->resize(static_cast<size_t>(head[0]));
  return t->empty() || static_cast<bool>(f.read(reinterpret_cast<char*>(t->data()), static_cast<std::streamsize>(sizeof(double) * 3 * t->size())));
}

std::string Slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

bool Exists(const std::string& path) { return static_cast<bool>(std::ifstream(path)); }

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 3 && std::strcmp(argv[1], "plan") == 0) {
    std::vector<std::array<double, 3>> t;
    smhip::MapPackageOptions o;
    EXPECT(ReadCase(argv[2], &t, &o));
    smhip::MapPackagePlan plan;
    std::string why;
    if (!smhip::PlanMapPackage(t, o, &plan, &why)) { std::printf("refused %s\n", why.c_str()); return 0; }
    std::printf("steps %d %d\n", plan.x_steps, plan.y_steps);
    for (int x = 0; x < plan.x_steps; ++x)
      for (int y = 0; y < plan.y_steps; ++y) {
        const smhip::MapPackagePiece& p = plan.Piece(x, y);
        std::printf("piece %d %d %.17g %.17g %.17g %.17g %.17g %.17g %zu", x, y, p.center[0], p.center[1], p.bb_min[0], p.bb_min[1], p.bb_max[0], p.bb_max[1],
                    p.inside_submaps.size());
        for (int m : p.inside_submaps) std::printf(" %d", m);
        std::printf("\n");
      }
    return 0;
  }
  if (argc >= 4 && std::strcmp(argv[1], "xml") == 0) {
    std::vector<std::array<double, 3>> t;
    smhip::MapPackageOptions o;
    EXPECT(ReadCase(argv[2], &t, &o));
    smhip::MapPackagePlan plan;
    EXPECT(smhip::PlanMapPackage(t, o, &plan));
    const std::string dir = argv[3];
    EXPECT(smhip::WriteMapPackageXml(dir + "/map_package.xml", plan, o));
    const std::string first = Slurp(dir + "/map_package.xml");
    EXPECT(smhip::WriteMapPackageXml(dir + "/map_package.xml", plan, o));
    EXPECT(!first.empty() && first == Slurp(dir + "/map_package.xml") && first == smhip::MapPackageXml(plan, o));
    EXPECT(!smhip::WriteMapPackageXml(dir + "/missing/map_package.xml", plan, o));
    EXPECT(!Exists(dir + "/missing/map_package.xml"));
    smhip::MapPackageOptions odd = o;
    odd.cloud_file_prefix = "a&b<c>\"d\n";
    EXPECT(smhip::MapPackageXml(plan, odd).find("file=\"a&amp;b&lt;c&gt;&quot;d&#10;0_0.pcd\" />") != std::string::npos);
    EXPECT(smhip::MapPackageXml(smhip::MapPackagePlan(), o) == "<?xml version=\"1.0\"?>\n<MapPackage />\n");
    // an empty piece's file: a valid header of 0 points and no rows
    EXPECT(smhip::SaveMapPackagePiece(dir + "/empty.pcd", nullptr, 0, false));
    EXPECT(Slurp(dir + "/empty.pcd") == smhip::pcd::BinaryHeader(0, false));
    std::printf("all checks passed\n");
    return 0;
  }
  if (argc >= 3 && std::strcmp(argv[1], "save") == 0) {
    const std::string dir = argv[2];
    std::vector<smhip::MapPackageSubmap> submaps(2);
    submaps[1].global_pose(0, 3) = 10.0;
    submaps[0].cloud.resize(4); submaps[1].cloud.resize(4);
    smhip::MapPackageOptions o;
    smhip::MapPackageResult r;
    EXPECT(!smhip::SaveTrajectoriesAsMapPackage(submaps, o, smhip::MrvmSettings(), dir + "/missing/", &r));
    EXPECT(!Exists(dir + "/missing/map_package.xml") && r.files.empty());
    o.piece_width = 0.0;                                          // refused before anything is written
    EXPECT(!smhip::SaveTrajectoriesAsMapPackage(submaps, o, smhip::MrvmSettings(), dir + "/", &r));
    EXPECT(!Exists(dir + "/map_package.xml"));
    o = smhip::MapPackageOptions();
    EXPECT(o.enable && o.border_offset == 100. && o.piece_width == 500. && o.cloud_file_prefix == "part_" && o.descript_filename == "map_package.xml");
    std::printf("all checks passed\n");
    return 0;
  }
  std::printf("usage: test_map_package plan IN | xml IN DIR | save DIR\n");
  return 2;
}
