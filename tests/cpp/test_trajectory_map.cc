// include/smhip/trajectory_map.h without a device: the map.xml reader and writer, the connection strings and the submap cloud files.
//   test_trajectory_map host TMPDIR          SubmapId, the connection strings, the pose conventions, cloud files of 0, 1 and 1 000 points
//   test_trajectory_map read FILE [BX BY]    ReadTrajectoryMap (against the base offset BX BY when given): one JSON line, "ok": false
//                                            with the reason when refused
//   test_trajectory_map rewrite FILE OUT     read FILE, write OUT beside it (so the submap files still resolve)
#define SMHIP_REGISTRATOR_THROW_ON_CHECK 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "smhip/trajectory_map.h"

namespace bld = smhip::builder;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static std::string Quoted(const std::string& s) {
  std::string o = "\"";
  for (char c : s) { if (c == '"' || c == '\\') o += '\\'; o += c; }
  return o + "\"";
}

static int Read(const char* file, const double* base) {
  bld::TrajectoryMap map;
  std::string why;
  if (!bld::ReadTrajectoryMap(file, &map, &why, base)) { std::printf("{\"ok\": false, \"why\": %s}\n", Quoted(why).c_str()); return 0; }
  std::printf("{\"ok\": true, \"base\": [%.17g, %.17g], \"trajectories\": [", map.base_x, map.base_y);
  for (size_t t = 0; t < map.trajectories.size(); ++t) {
    const bld::MapTrajectory& tr = map.trajectories[t];
    std::printf("%s{\"id\": %d, \"offset\": [%.17g, %.17g], \"submaps\": [", t ? ", " : "", tr.id, tr.offset_x, tr.offset_y);
    for (size_t k = 0; k < tr.submaps.size(); ++k) {
      const bld::MapSubmap& s = tr.submaps[k];
      std::printf("%s{\"id\": [%d, %d], \"debug\": %s, \"file\": %s, \"path\": %s, \"pose6\": [", k ? ", " : "", s.id.trajectory_index, s.id.submap_index,
                  Quoted(s.id.DebugString()).c_str(), Quoted(s.file).c_str(), Quoted(s.Path()).c_str());
      for (int c = 0; c < 6; ++c) std::printf("%s%.17g", c ? ", " : "", s.pose6[c]);
      std::printf("], \"pose\": [");
      for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) std::printf("%s%.17g", (r || c) ? ", " : "", s.pose(r, c));
      std::printf("], \"connections\": [");
      for (size_t c = 0; c < s.connections.size(); ++c) std::printf("%s[%d, %d]", c ? ", " : "", s.connections[c].trajectory_index, s.connections[c].submap_index);
      std::printf("]}");
    }
    std::printf("]}");
  }
  std::printf("]}\n");
  return 0;
}

static void Strings() {
  bld::SubmapId id;
  id.trajectory_index = 2; id.submap_index = 17;
  EXPECT(id.DebugString() == "(2,17)");
  bld::SubmapId other = id;
  EXPECT(other == id && !(other < id));
  other.submap_index = 3;
  EXPECT(other != id && other < id);
  other.trajectory_index = 3;
  EXPECT(id < other);
  EXPECT(bld::ConnectionsStrToIds("").empty());
  const std::vector<bld::SubmapId> ids = bld::ConnectionsStrToIds("[0,63][0,80][12,5]");
  EXPECT(ids.size() == 3 && ids[0].trajectory_index == 0 && ids[0].submap_index == 63 && ids[1].submap_index == 80 && ids[2].trajectory_index == 12 && ids[2].submap_index == 5);
  EXPECT(bld::ConnectionsIdsToStr(ids) == "[0,63][0,80][12,5]" && bld::ConnectionsIdsToStr({}) == "");
  EXPECT(bld::ConnectionsStrToIds("[0,1]").size() == 1);
  EXPECT(bld::FilePath("a/b/map.xml") == "a/b/" && bld::FilePath("map.xml") == "./" && bld::FilePath("/map.xml") == "/");
}

static void Poses() {
  // R = Rz Ry Rx: a quarter turn about z takes x to y; about x takes y to z
  const double z90[6] = {1, 2, 3, 0, 0, M_PI / 2}, x90[6] = {0, 0, 0, M_PI / 2, 0, 0};
  const bld::Matrix4d Z = bld::Vector6ToTransform(z90), X = bld::Vector6ToTransform(x90);
  EXPECT(std::fabs(Z(1, 0) - 1) < 1e-15 && std::fabs(Z(0, 1) + 1) < 1e-15 && Z(0, 3) == 1 && Z(1, 3) == 2 && Z(2, 3) == 3 && Z(3, 3) == 1);
  EXPECT(std::fabs(X(2, 1) - 1) < 1e-15 && std::fabs(X(1, 2) + 1) < 1e-15);
  const double v[6] = {-3.5, 0.25, 8, 0.1, -0.2, 2.9};
  double back[6];
  bld::TransformToVector6(bld::Vector6ToTransform(v), back);
  for (int c = 0; c < 6; ++c) EXPECT(std::fabs(back[c] - v[c]) < 1e-14);
  // SetPose leaves what a reader of the written file gets: the six numbers and their matrix
  bld::MapSubmap s;
  s.SetPose(bld::Vector6ToTransform(v));
  const bld::Matrix4d again = bld::Vector6ToTransform(s.pose6);
  EXPECT(std::memcmp(again.data(), s.pose.data(), sizeof(double) * 16) == 0);
}

static void Clouds(const std::string& dir) {
  for (int n : {0, 1, 1000}) {
    smhip::data::InnerCloudType cloud, back;
    cloud.stamp = 1234567890123456789ll % 4000000000000000000ll;
    for (int k = 0; k < n; ++k) {
      smhip::data::InnerPointType p;
      p.x = 0.5f * k; p.y = -1.25f + k; p.z = 1.0f / (k + 1); p.intensity = static_cast<float>(k % 256); p.factor = k / 1000.0f;
      cloud.points.push_back(p);
    }
    const std::string file = dir + "/cloud_" + std::to_string(n) + ".bin";
    std::string why;
    EXPECT(bld::WriteSubmapCloud(file, cloud, &why));
    FILE* f = std::fopen(file.c_str(), "rb");
    EXPECT(f != nullptr);
    if (!f) continue;
    std::vector<unsigned char> raw(20 + 20 * static_cast<size_t>(n) + 1);
    const size_t got = std::fread(raw.data(), 1, raw.size(), f);
    std::fclose(f);
    EXPECT(got == 20 + 20 * static_cast<size_t>(n));                      // 12 + 8 + 20 n bytes, nothing between them
    uint32_t head[3]; uint64_t count;
    std::memcpy(head, raw.data(), 12); std::memcpy(&count, raw.data() + 12, 8);
    EXPECT(head[0] == static_cast<uint32_t>(cloud.stamp / 1000000000ll) && head[1] == static_cast<uint32_t>(cloud.stamp % 1000000000ll) && head[2] == 1u && count == static_cast<uint64_t>(n));
    if (n > 0) { float x1[5]; std::memcpy(x1, raw.data() + 20 + 20 * static_cast<size_t>(n - 1), 20); EXPECT(x1[0] == cloud.points.back().x && x1[4] == cloud.points.back().factor); }
    EXPECT(bld::ReadSubmapCloud(file, &back, &why));
    EXPECT(back.stamp == cloud.stamp && back.points.size() == cloud.points.size());
    EXPECT(n == 0 || std::memcmp(back.points.data(), cloud.points.data(), 20 * static_cast<size_t>(n)) == 0);
    if (n == 1000) {                                                       // a cut file and a count that does not fit are refused, not read short
      f = std::fopen((file + ".cut").c_str(), "wb");
      std::fwrite(raw.data(), 1, got - 7, f);
      std::fclose(f);
      EXPECT(!bld::ReadSubmapCloud(file + ".cut", &back, &why) && why.find("is not 20 + 20 x its count of 1000") != std::string::npos);
    }
  }
  smhip::data::InnerCloudType back;
  std::string why;
  EXPECT(!bld::ReadSubmapCloud(dir + "/none.bin", &back, &why) && why.find("does not exist") != std::string::npos);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "host" && argc == 3) {
    Strings();
    Poses();
    Clouds(argv[2]);
    std::printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
  }
  if (mode == "read" && (argc == 3 || argc == 5)) {
    double base[2] = {0, 0};
    if (argc == 5) { base[0] = std::atof(argv[3]); base[1] = std::atof(argv[4]); }
    return Read(argv[2], argc == 5 ? base : nullptr);
  }
  if (mode == "rewrite" && argc == 4) {
    bld::TrajectoryMap map;
    std::string why;
    if (!bld::ReadTrajectoryMap(argv[2], &map, &why) || !bld::WriteTrajectoryMap(argv[3], map, &why)) { std::fprintf(stderr, "%s\n", why.c_str()); return 1; }
    return 0;
  }
  std::fprintf(stderr, "usage: test_trajectory_map host TMPDIR | read FILE [BX BY] | rewrite FILE OUT\n");
  return 2;
}
