// smhip/map_package.h -- static_map::SaveTrajectoriesAsMapPackage (the reference's builder/map_package.{h,cc}, called from
// MapBuilder::SaveMapPackage, builder/map_builder.cc:816-823): the static map cut into overlapping square pieces, one PCD file per
// piece centred on the piece, and an XML file that lists them -- the artefact a localiser loads.  Header-only; link with -lsmhip.
//
//   plan     map_package.cc:59-141   PlanMapPackage (smhip_map_package_plan, host only): the extent of the submaps' translations
//                                    widened by border_offset, pieces piece_width wide and piece_width / 2 apart, each with the
//                                    submaps whose translation lies in its box widened by border_offset
//   fill     :143-184                a fresh voxel map per piece; a member submap whose translation lies in the box goes in whole
//                                    (smhip_mrvm_insert_transformed_f32), any other only with the rows whose transformed x, y lie
//                                    in the box (smhip_mrvm_insert_transformed_clipped_f32); no row kept, no insert
//   cut      :186-198                OutputToPointCloud(prob_threshold), the rows inside the box, moved to the piece's centre
//                                    (smhip_mrvm_output_clipped)
//   files    :200-227                <cloud_file_prefix><x>_<y>.pcd for every piece, <descript_filename> with one Piece element
//                                    per piece, x-major, doubles as pugixml 1.9 writes them (%.17g), pugixml's default layout
//
// What differs from the reference, on purpose:
//   * refused before any work: a piece_width that is not finite and positive, a border_offset that is not finite, more than
//     65 536 pieces (the reference would divide by zero or overflow a stack array), no submap, a translation that is not finite;
//   * a piece file is DATA binary like the static map's (smhip/pcd.h); binary_compressed, the reference's format here, is not written;
//   * the rows of a piece are in voxel-key order (SMHIP_MRVM_SORTED), so a package is the same bytes on every run;
//   * a piece with no rows is a valid PCD file of 0 points (PCL refuses to write one);
//   * one voxel map is emptied and used again for every piece (smhip_mrvm_clear) instead of a new one per piece;
//   * output_rgb of the settings is honoured (the reference's package is always PointXYZI);
//   * when anything fails the files this call wrote are removed: there is no partial package;
//   * one trajectory; GenerateMapPackage's map.xml of trajectories is not written.
#ifndef SMHIP_MAP_PACKAGE_H_
#define SMHIP_MAP_PACKAGE_H_

#include <algorithm>
#include <array>
#include <cstdio>
#include <string>
#include <vector>

#include "../smhip.h"
#include "mrvm.h"
#include "pcd.h"
#include "registrator.h"

namespace smhip {

struct MapPackageOptions {                    // builder/map_package.h:36-41
  bool enable = true;
  double border_offset = 100.;
  double piece_width = 500.;
  std::string cloud_file_prefix = "part_";
  std::string descript_filename = "map_package.xml";
};

struct MapPackagePiece {                      // SeperatedPart, map_package.cc:35-49
  double center[2] = {0., 0.}, bb_min[2] = {0., 0.}, bb_max[2] = {0., 0.};
  std::vector<int> inside_submaps;            // indices into the submap list, ascending
};
struct MapPackagePlan {
  int x_steps = 0, y_steps = 0;
  std::vector<MapPackagePiece> pieces;        // piece (x, y) at x * y_steps + y
  const MapPackagePiece& Piece(int x, int y) const { return pieces.at(static_cast<size_t>(x) * y_steps + y); }
};

// A submap as builder::Submap holds it after a download: its global pose and its cloud in its own (first frame's) coordinates.
struct MapPackageSubmap {
  registrator::Matrix4d global_pose = registrator::Matrix4d::Identity();
  std::vector<data::InnerPointType> cloud;
};

// map_package.cc:59-141.  translations: Submap::GlobalTranslation of every submap, in trajectory order.  false: refused, the reason
// in *why.  No device involved.
inline bool PlanMapPackage(const std::vector<std::array<double, 3>>& translations, const MapPackageOptions& options, MapPackagePlan* plan,
                           std::string* why = nullptr) {
  SMHIP_CHECK(plan != nullptr, "PlanMapPackage: null plan");
  *plan = MapPackagePlan();
  smhip_map_package_options o;
  smhip_map_package_default_options(&o);
  o.border_offset = options.border_offset; o.piece_width = options.piece_width;
  const int n = static_cast<int>(translations.size());
  const double* t = n > 0 ? translations[0].data() : nullptr;
  char reason[160] = "";
  int32_t steps[2] = {0, 0}, n_members = 0;
  if (smhip_map_package_plan(n, t, &o, steps, 0, nullptr, nullptr, nullptr, 0, nullptr, &n_members, reason, sizeof(reason)) != SMHIP_OK) {
    if (why) *why = reason;
    return false;
  }
  const size_t P = static_cast<size_t>(steps[0]) * steps[1];
  std::vector<double> centres(2 * P), boxes(4 * P);
  std::vector<int32_t> offsets(P + 1), members(static_cast<size_t>(n_members) + 1);
  if (smhip_map_package_plan(n, t, &o, steps, static_cast<int>(P), centres.data(), boxes.data(), offsets.data(), n_members, members.data(), &n_members,
                             reason, sizeof(reason)) != SMHIP_OK) {
    if (why) *why = reason;
    return false;
  }
  plan->x_steps = steps[0]; plan->y_steps = steps[1];
  plan->pieces.resize(P);
  for (size_t i = 0; i < P; ++i) {
    MapPackagePiece& p = plan->pieces[i];
    p.center[0] = centres[2 * i]; p.center[1] = centres[2 * i + 1];
    p.bb_min[0] = boxes[4 * i]; p.bb_min[1] = boxes[4 * i + 1]; p.bb_max[0] = boxes[4 * i + 2]; p.bb_max[1] = boxes[4 * i + 3];
    p.inside_submaps.assign(members.begin() + offsets[i], members.begin() + offsets[i + 1]);
  }
  return true;
}

inline std::string MapPackagePieceFile(const MapPackageOptions& options, int x, int y) {              // :201-203
  return options.cloud_file_prefix + std::to_string(x) + "_" + std::to_string(y) + ".pcd";
}

// The description file's text (:211-227) as pugixml 1.9 writes it with its defaults: the declaration, a tab per level, one element
// per line, attributes x, y (set from a double: "%.17g") and file, an empty element closed by " />".  Attribute values are escaped
// as pugixml escapes them (& < > " and control characters).
inline std::string MapPackageXml(const MapPackagePlan& plan, const MapPackageOptions& options) {
  auto escaped = [](const std::string& s) {
    std::string out;
    for (const char ch : s) {
      const unsigned char c = static_cast<unsigned char>(ch);
      if (ch == '&') out += "&amp;";
      else if (ch == '<') out += "&lt;";
      else if (ch == '>') out += "&gt;";
      else if (ch == '"') out += "&quot;";
      else if (c < 32 && ch != '\t') { out += "&#"; out += static_cast<char>('0' + c / 10); out += static_cast<char>('0' + c % 10); out += ';'; }
      else out += ch;
    }
    return out;
  };
  auto number = [](double v) { char buf[128]; std::snprintf(buf, sizeof(buf), "%.17g", v); return std::string(buf); };
  std::string text = "<?xml version=\"1.0\"?>\n";
  if (plan.pieces.empty()) return text + "<MapPackage />\n";
  text += "<MapPackage>\n";
  for (int x = 0; x < plan.x_steps; ++x)
    for (int y = 0; y < plan.y_steps; ++y) {
      const MapPackagePiece& p = plan.Piece(x, y);
      text += "\t<Piece x=\"" + number(p.center[0]) + "\" y=\"" + number(p.center[1]) + "\" file=\"" + escaped(MapPackagePieceFile(options, x, y)) + "\" />\n";
    }
  return text + "</MapPackage>\n";
}

namespace map_package_detail {
inline bool WriteWhole(const std::string& path, const void* a, size_t na, const void* b, size_t nb) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) { std::fprintf(stderr, "[ERROR] cannot write %s\n", path.c_str()); return false; }
  bool ok = (na == 0 || std::fwrite(a, 1, na, f) == na) && (nb == 0 || std::fwrite(b, 1, nb, f) == nb);
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) { std::fprintf(stderr, "[ERROR] short write to %s\n", path.c_str()); std::remove(path.c_str()); }
  return ok;
}
}  // namespace map_package_detail

// false: the file cannot be written (nothing is left behind)
inline bool WriteMapPackageXml(const std::string& path, const MapPackagePlan& plan, const MapPackageOptions& options) {
  const std::string text = MapPackageXml(plan, options);
  return map_package_detail::WriteWhole(path, text.data(), text.size(), nullptr, 0);
}

// A piece's file: smhip/pcd.h's layout, n = 0 included (a header with WIDTH 0 and POINTS 0, no rows).
inline bool SaveMapPackagePiece(const std::string& path, const float* rows, size_t n, bool rgb) {
  const std::string h = pcd::BinaryHeader(n, rgb);
  return map_package_detail::WriteWhole(path, h.data(), h.size(), rows, n * 4 * sizeof(float));
}

struct MapPackageResult {
  int pieces = 0, submaps = 0;
  long long points = 0, inserts = 0, clipped_inserts = 0;
  std::vector<std::string> files;             // every file written, the description last
};

// map_package.cc:51-230 for one trajectory.  export_path is joined to the file names as it is, like the reference does (give it
// its trailing '/').  intensity_scale: what a row's 4th float is multiplied by on its way into the map (255 for clouds made of raw
// KITTI rows, whose reader the reference lets scale them, kitti_reader.cc:113).  false: refused, or a file could not be written, or
// the device refused an insert (the reason on stderr); the files of this call are then removed.
inline bool SaveTrajectoriesAsMapPackage(const std::vector<MapPackageSubmap>& submaps, const MapPackageOptions& map_package_options,
                                         const MrvmSettings& mrvm_options, const std::string& export_path, MapPackageResult* result = nullptr,
                                         int device = 0, float intensity_scale = 1.f, int max_table_log2 = 28) {
  MapPackageResult res;
  res.submaps = static_cast<int>(submaps.size());
  std::vector<std::array<double, 3>> translations(submaps.size());
  size_t max_cloud = 1;
  for (size_t i = 0; i < submaps.size(); ++i) {
    translations[i] = {submaps[i].global_pose(0, 3), submaps[i].global_pose(1, 3), submaps[i].global_pose(2, 3)};
    max_cloud = std::max(max_cloud, submaps[i].cloud.size());
  }
  MapPackagePlan plan;
  std::string why;
  if (!PlanMapPackage(translations, map_package_options, &plan, &why)) {
    std::fprintf(stderr, "[WARNING] map package refused: %s\n", why.c_str());
    return false;
  }
  // the description's place is taken first: a directory that is missing or cannot be written ends the call before any device work
  const std::string descript = export_path + map_package_options.descript_filename;
  if (!map_package_detail::WriteWhole(descript, nullptr, 0, nullptr, 0)) return false;
  std::vector<std::string> written(1, descript);
  auto fail = [&written]() { for (const std::string& f : written) std::remove(f.c_str()); return false; };

  smhip_mrvm_settings s;
  smhip_mrvm_default_settings(&s);
  s.prob_threshold = mrvm_options.prob_threshold; s.high_resolution = mrvm_options.high_resolution; s.hit_prob = mrvm_options.hit_prob;
  s.miss_prob = mrvm_options.miss_prob; s.z_offset = mrvm_options.z_offset; s.max_point_num_in_cell = mrvm_options.max_point_num_in_cell;
  s.use_max_intensity = mrvm_options.use_max_intensity ? 1 : 0;
  smhip_mrvm_handle h = nullptr;
  const smhip_status created = smhip_mrvm_create(device, std::min(22, max_table_log2), static_cast<int>(max_cloud), &s, &h);
  if (created != SMHIP_OK) {
    std::fprintf(stderr, "[ERROR] smhip_mrvm_create: %s (no gfx950 device? there is no CPU fallback)\n", smhip_status_string(created));
    return fail();
  }
  bool ok = smhip_mrvm_set_max_table_log2(h, max_table_log2) == SMHIP_OK;
  const int flags = (mrvm_options.output_average ? SMHIP_MRVM_AVERAGE : 0) | (mrvm_options.output_rgb ? SMHIP_MRVM_RGB : 0);
  static_assert(sizeof(data::InnerPointType) == 5 * sizeof(float), "InnerPointType is five floats");
  std::vector<float> rows;
  for (int x = 0; ok && x < plan.x_steps; ++x) {
    for (int y = 0; ok && y < plan.y_steps; ++y) {
      const MapPackagePiece& part = plan.Piece(x, y);
      if (x + y > 0) ok = smhip_mrvm_clear(h) == SMHIP_OK;                                           // a fresh map, :149-150
      for (size_t k = 0; ok && k < part.inside_submaps.size(); ++k) {
        const MapPackageSubmap& submap = submaps[static_cast<size_t>(part.inside_submaps[k])];
        if (submap.cloud.empty()) continue;                                                          // InsertPointCloud: "cloud is empty."
        const int n = static_cast<int>(submap.cloud.size());
        const double px = submap.global_pose(0, 3), py = submap.global_pose(1, 3);
        smhip_status st;
        if (px >= part.bb_min[0] && px <= part.bb_max[0] && py >= part.bb_min[1] && py <= part.bb_max[1]) {   // :162-166
          st = smhip_mrvm_insert_transformed_f32(h, &submap.cloud[0].x, 5, n, submap.global_pose.data(), intensity_scale);
          ++res.inserts;
        } else {                                                                                     // :167-182
          int kept = 0;
          st = smhip_mrvm_insert_transformed_clipped_f32(h, &submap.cloud[0].x, 5, n, submap.global_pose.data(), intensity_scale, part.bb_min,
                                                         part.bb_max, &kept);
          if (kept > 0) { ++res.inserts; ++res.clipped_inserts; }
        }
        if (st != SMHIP_OK) {
          std::fprintf(stderr, "[ERROR] map package: piece %d_%d refused submap %d: %s\n", x, y, part.inside_submaps[k], smhip_mrvm_last_error(h));
          ok = false;
        } else if (smhip_mrvm_last_error(h)[0]) {
          std::fprintf(stderr, "[WARNING] map package: piece %d_%d, submap %d: %s\n", x, y, part.inside_submaps[k], smhip_mrvm_last_error(h));
        }
      }
      if (!ok) break;
      int n = 0, m = 0;                                                                              // :186-198
      ok = smhip_mrvm_output_clipped(h, mrvm_options.prob_threshold, flags, part.bb_min, part.bb_max, part.center, nullptr, 0, &n) == SMHIP_OK;
      rows.resize(4 * static_cast<size_t>(std::max(n, 0)));
      if (ok && n > 0) ok = smhip_mrvm_output_clipped(h, mrvm_options.prob_threshold, flags, part.bb_min, part.bb_max, part.center, rows.data(), n, &m) == SMHIP_OK && m == n;
      if (!ok) { std::fprintf(stderr, "[ERROR] map package: output of piece %d_%d: %s\n", x, y, smhip_mrvm_last_error(h)); break; }
      const std::string file = export_path + MapPackagePieceFile(map_package_options, x, y);
      written.push_back(file);
      ok = SaveMapPackagePiece(file, rows.data(), static_cast<size_t>(n), mrvm_options.output_rgb);
      res.points += n;
      ++res.pieces;
    }
  }
  smhip_mrvm_destroy(h);
  ok = ok && WriteMapPackageXml(descript, plan, map_package_options);                               // :210-227
  if (!ok) return fail();
  res.files.assign(written.begin() + 1, written.end());
  res.files.push_back(descript);
  if (result) *result = res;
  return true;
}

}  // namespace smhip
#endif  // SMHIP_MAP_PACKAGE_H_
