// smhip/trajectory_map.h -- the files a finished map is kept in, so that a second drive can be joined to it: the reference's map.xml
// (builder/trajectory.cc:32-58 writes it, builder/multi_trajectory/multi_trajectory_map_builder.cc:140-212 reads it) and its submap
// cloud files (builder/data/cloud_types.cc:180-230).  Header-only; nothing here touches a device.
//
//   SubmapId, DebugString                builder/submap.cc:55-64
//   ConnectionsStrToIds                  multi_trajectory_map_builder.cc:277-299     "[0,63][0,80]" -> ids; "" -> none
//   ConnectionsIdsToStr                  trajectory.cc:49-56                         its inverse
//   Vector6ToTransform                   common/math.h:163-174                       (tx ty tz rx ry rz) -> pose, R = Rz Ry Rx
//   TransformToVector6                   common/math.h:153-160                       its inverse (RotationMatrixToEulerAngles, :108-127)
//   ReadTrajectoryMap                    LoadTrajectoryFromFile, :140-212
//   WriteTrajectoryMap                   SaveWholeMap, :214-228, over Trajectory::ToXmlNode, trajectory.cc:32-58
//   WriteSubmapCloud / ReadSubmapCloud   InnerCloudType::Serialize / Deserialize, cloud_types.cc:180-230
//
// The file:   <Map> <Trajectory id enu_x enu_y> <Submap id file tx ty tz rx ry rz connections /> ... </Trajectory> ... </Map>
// pugixml is replaced by a reader for exactly this shape: elements with double-quoted attributes, the XML declaration, comments and
// the five predefined entities; no text nodes, CDATA or DOCTYPE.
//
// AN INCONSISTENCY OF THE REFERENCE, kept visible: a trajectory's offset pair is WRITTEN as enu_x / enu_y (trajectory.cc:35-36) and
// READ as utm_x / utm_y (multi_trajectory_map_builder.cc:169-173), so a file the reference wrote reads back with offsets of 0.  Here
// utm_* is read when present, else enu_*, else 0, and enu_* is written, as the reference writes it.  The first trajectory of the base
// map defines the base offset; every trajectory's tx, ty get its own offset minus the base offset (:172-173, 187-188), and every
// trajectory is written with the base offset (:223), since its poses are then in the base map's frame.
//
// Numbers are written as %.17g and a submap keeps the six numbers it was read with until SetPose replaces them, so a file that is
// read and written again keeps every bit, and so does a file that is written and read.
//
// The cloud file, by explicit field sizes (little-endian, no padding: the reference writes the three parts one after the other):
//   12 bytes  SimpleTime: u32 secs, u32 nsecs, u32 u_judge_range (always 1; common/simple_time.h:101-110)
//    8 bytes  u64 point count (size_t)
//   20 bytes  per point: f32 x, y, z, intensity, factor (InnerPointType, cloud_types.h:46-51)
// InnerCloudType::stamp here is in nanoseconds (SimpleTime::ToNanoSec).
#ifndef SMHIP_TRAJECTORY_MAP_H_
#define SMHIP_TRAJECTORY_MAP_H_

#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "smhip/back_end.h"

namespace smhip {
namespace builder {

using registrator::Matrix4d;

struct SubmapId {
  int32_t trajectory_index = 0;
  int32_t submap_index = 0;
  bool operator==(const SubmapId& o) const { return trajectory_index == o.trajectory_index && submap_index == o.submap_index; }
  bool operator!=(const SubmapId& o) const { return !(*this == o); }
  bool operator<(const SubmapId& o) const {
    return trajectory_index != o.trajectory_index ? trajectory_index < o.trajectory_index : submap_index < o.submap_index;
  }
  std::string DebugString() const { return "(" + std::to_string(trajectory_index) + "," + std::to_string(submap_index) + ")"; }
};

// "[0,63][0,80]" -> {(0,63), (0,80)}: split at ']', the first number after '[', the second after ','
inline std::vector<SubmapId> ConnectionsStrToIds(const std::string& connections) {
  std::vector<SubmapId> ids;
  if (connections.empty()) return ids;
  std::stringstream ss(connections);
  std::string token;
  while (std::getline(ss, token, ']')) {
    const size_t open = token.find('['), comma = token.find(',');
    if (open == std::string::npos || comma == std::string::npos || open + 1 > comma) continue;   // (the reference CHECKs; a stray tail is skipped)
    SubmapId id;
    id.trajectory_index = std::atoi(token.substr(open + 1, comma - open - 1).c_str());
    id.submap_index = std::atoi(token.substr(comma + 1).c_str());
    ids.push_back(id);
  }
  return ids;
}
inline std::string ConnectionsIdsToStr(const std::vector<SubmapId>& ids) {
  std::string s;
  for (const SubmapId& id : ids) s += "[" + std::to_string(id.trajectory_index) + "," + std::to_string(id.submap_index) + "]";
  return s;
}

// common::Vector6ToTransform: the translation, then R = Rz(rz) Ry(ry) Rx(rx)
inline Matrix4d Vector6ToTransform(const double v[6]) {
  const double cx = std::cos(v[3]), sx = std::sin(v[3]), cy = std::cos(v[4]), sy = std::sin(v[4]), cz = std::cos(v[5]), sz = std::sin(v[5]);
  Matrix4d tf = Matrix4d::Identity();
  tf(0, 0) = cz * cy; tf(0, 1) = cz * sy * sx - sz * cx; tf(0, 2) = cz * sy * cx + sz * sx;
  tf(1, 0) = sz * cy; tf(1, 1) = sz * sy * sx + cz * cx; tf(1, 2) = sz * sy * cx - cz * sx;
  tf(2, 0) = -sy;     tf(2, 1) = cy * sx;                tf(2, 2) = cy * cx;
  for (int c = 0; c < 3; ++c) tf(c, 3) = v[c];
  return tf;
}
inline void TransformToVector6(const Matrix4d& t, double v[6]) {
  for (int c = 0; c < 3; ++c) v[c] = t(c, 3);
  back_end::RotationMatrixToEulerAngles(t, v + 3);
}

// The same pose without a negative zero among its entries (x + 0.0).  Vector6ToTransform leaves -0.0 where an angle is 0 (-sin(0));
// Eigen's route through a quaternion, which the reference takes, does not.  A pose without one is a fixed point of the pose graph's
// retraction by a zero step (R * I, t + R * 0, whose sums of zeros come out positive), so a map that is loaded and solved at its
// optimum keeps every bit.
inline Matrix4d WithoutNegativeZero(Matrix4d t) {
  for (int q = 0; q < 16; ++q) t.data()[q] += 0.0;
  return t;
}

struct MapSubmap {
  SubmapId id;
  std::string file;                       // as in the xml: relative to `dir`, or an absolute path
  std::string dir;                        // the xml's directory, with its trailing '/' (Submap::SetSavePath)
  double pose6[6] = {0, 0, 0, 0, 0, 0};   // tx ty tz rx ry rz in the base map's frame: what the writer writes
  Matrix4d pose = Matrix4d::Identity();   // WithoutNegativeZero(Vector6ToTransform(pose6))
  std::vector<SubmapId> connections;
  std::string Path() const { return !file.empty() && file[0] == '/' ? file : dir + file; }
  // a pose from a solve: held as the six numbers the file will carry, and as the matrix a reader of that file gets
  void SetPose(const Matrix4d& p) { TransformToVector6(p, pose6); pose = WithoutNegativeZero(Vector6ToTransform(pose6)); }
};

struct MapTrajectory {
  int id = 0;
  double offset_x = 0.0, offset_y = 0.0;  // as read (utm_* or enu_*)
  std::vector<MapSubmap> submaps;
};

struct TrajectoryMap {
  double base_x = 0.0, base_y = 0.0;      // the first trajectory's offset pair of the base map
  std::vector<MapTrajectory> trajectories;
  size_t SubmapCount() const { size_t n = 0; for (const MapTrajectory& t : trajectories) n += t.submaps.size(); return n; }
};

inline std::string FilePath(const std::string& file) {                    // common::FilePath: up to and with the last '/'
  const size_t slash = file.find_last_of('/');
  return slash == std::string::npos ? std::string("./") : file.substr(0, slash + 1);
}
inline bool FileExist(const std::string& file) { std::ifstream f(file, std::ios::binary); return f.good(); }

namespace xml {
struct Element {
  std::string name;
  std::vector<std::pair<std::string, std::string>> attributes;
  std::vector<Element> children;
  const std::string* Find(const char* key) const {
    for (const auto& a : attributes) if (a.first == key) return &a.second;
    return nullptr;
  }
};
inline std::string Decode(const std::string& s) {
  std::string out;
  for (size_t i = 0; i < s.size(); ++i) {
    if (s[i] != '&') { out += s[i]; continue; }
    static const char* const from[] = {"&quot;", "&amp;", "&lt;", "&gt;", "&apos;"};
    static const char to[] = {'"', '&', '<', '>', '\''};
    bool hit = false;
    for (int k = 0; k < 5 && !hit; ++k) {
      const size_t len = std::strlen(from[k]);
      if (s.compare(i, len, from[k]) == 0) { out += to[k]; i += len - 1; hit = true; }
    }
    if (!hit) out += s[i];
  }
  return out;
}
inline std::string Encode(const std::string& s) {
  std::string out;
  for (char c : s) {
    if (c == '"') out += "&quot;"; else if (c == '&') out += "&amp;"; else if (c == '<') out += "&lt;"; else if (c == '>') out += "&gt;"; else out += c;
  }
  return out;
}
// The top-level elements of `text` into root->children.  false with `why` on anything outside the shape named at the top.
inline bool Parse(const std::string& text, Element* root, std::string* why) {
  std::vector<Element*> open{root};
  size_t at = 0;
  auto is_name = [](char c) { return std::isalnum(static_cast<unsigned char>(c)) || c == '_' || c == '-' || c == ':' || c == '.'; };
  auto skip_space = [&]() { while (at < text.size() && std::isspace(static_cast<unsigned char>(text[at]))) ++at; };
  auto fail = [&](const std::string& what) { *why = what + " at byte " + std::to_string(at); return false; };
  for (;;) {
    skip_space();
    if (at >= text.size()) break;
    if (text[at] != '<') return fail("text outside an element");
    if (text.compare(at, 2, "<?") == 0) { const size_t e = text.find("?>", at); if (e == std::string::npos) return fail("unterminated declaration"); at = e + 2; continue; }
    if (text.compare(at, 4, "<!--") == 0) { const size_t e = text.find("-->", at); if (e == std::string::npos) return fail("unterminated comment"); at = e + 3; continue; }
    if (text.compare(at, 2, "</") == 0) {
      at += 2;
      const size_t b = at;
      while (at < text.size() && is_name(text[at])) ++at;
      if (open.size() < 2 || text.substr(b, at - b) != open.back()->name) return fail("a closing tag that closes nothing");
      skip_space();
      if (at >= text.size() || text[at] != '>') return fail("a closing tag without '>'");
      ++at;
      open.pop_back();
      continue;
    }
    ++at;
    const size_t b = at;
    while (at < text.size() && is_name(text[at])) ++at;
    if (at == b) return fail("an element without a name");
    Element el;
    el.name = text.substr(b, at - b);
    bool closed = false;
    for (;;) {
      skip_space();
      if (at >= text.size()) return fail("an unterminated element");
      if (text[at] == '>') { ++at; break; }
      if (text.compare(at, 2, "/>") == 0) { at += 2; closed = true; break; }
      const size_t kb = at;
      while (at < text.size() && is_name(text[at])) ++at;
      if (at == kb) return fail("an attribute without a name");
      const std::string key = text.substr(kb, at - kb);
      skip_space();
      if (at >= text.size() || text[at] != '=') return fail("an attribute without '='");
      ++at;
      skip_space();
      if (at >= text.size() || text[at] != '"') return fail("an attribute value without double quotes");
      const size_t e = text.find('"', at + 1);
      if (e == std::string::npos) return fail("an unterminated attribute value");
      el.attributes.emplace_back(key, Decode(text.substr(at + 1, e - at - 1)));
      at = e + 1;
    }
    open.back()->children.push_back(std::move(el));
    if (!closed) open.push_back(&open.back()->children.back());    // (stays valid: nothing is appended to the parent while it is open)
  }
  if (open.size() != 1) return fail("an element that is never closed");
  return true;
}
}  // namespace xml

// LoadTrajectoryFromFile: the trajectories of `file` in `out`, indexed from 0, connections as the file names them.  `base_offset`
// null: the file is a base map and its first trajectory defines out->base_x / base_y (update_base_utm); else the pair every
// trajectory's offset is taken against.  false with the reason in `why` (and `out` untouched): a missing file, no <Map>, a submap
// file that does not exist, submap ids that are not 0..n-1 in order (multi_trajectory_optimizer.cc:122 indexes by them), a
// connection naming a submap that does not exist, a number that does not parse.
inline bool ReadTrajectoryMap(const std::string& file, TrajectoryMap* out, std::string* why, const double* base_offset = nullptr) {
  std::string sink;
  if (!why) why = &sink;
  std::ifstream in(file, std::ios::binary);
  if (!in) { *why = "map file does not exist: " + file; return false; }
  std::stringstream buffer;
  buffer << in.rdbuf();
  xml::Element root;
  std::string parse_why;
  if (!xml::Parse(buffer.str(), &root, &parse_why)) { *why = "map file " + file + " is not the xml this reader takes: " + parse_why; return false; }
  const xml::Element* map_node = nullptr;
  for (const xml::Element& e : root.children) if (e.name == "Map") { map_node = &e; break; }
  if (!map_node) { *why = "no <Map> element in " + file; return false; }
  auto number = [&](const xml::Element& e, const char* key, double* v) {
    const std::string* s = e.Find(key);
    if (!s) { *v = 0.0; return true; }                                   // pugixml's as_double of a missing attribute
    char* end = nullptr;
    *v = std::strtod(s->c_str(), &end);
    if (end == s->c_str() || *end != '\0' || !std::isfinite(*v)) { *why = std::string("attribute ") + key + "=\"" + *s + "\" of <" + e.name + "> in " + file + " is not a finite number"; return false; }
    return true;
  };
  TrajectoryMap m;
  const std::string dir = FilePath(file);
  for (const xml::Element& t_node : map_node->children) {
    if (t_node.name != "Trajectory") continue;
    MapTrajectory t;
    t.id = static_cast<int>(m.trajectories.size());
    const bool utm = t_node.Find("utm_x") || t_node.Find("utm_y");
    if (!number(t_node, utm ? "utm_x" : "enu_x", &t.offset_x) || !number(t_node, utm ? "utm_y" : "enu_y", &t.offset_y)) return false;
    if (m.trajectories.empty()) {
      if (base_offset) { m.base_x = base_offset[0]; m.base_y = base_offset[1]; }
      else { m.base_x = t.offset_x; m.base_y = t.offset_y; }
    }
    const double dx = t.offset_x - m.base_x, dy = t.offset_y - m.base_y;
    for (const xml::Element& s_node : t_node.children) {
      if (s_node.name != "Submap") continue;
      MapSubmap s;
      s.id.trajectory_index = t.id;
      double id = 0.0;
      if (!number(s_node, "id", &id)) return false;
      s.id.submap_index = static_cast<int32_t>(id);
      if (s.id.submap_index != static_cast<int32_t>(t.submaps.size()) || id != s.id.submap_index) {
        *why = "submap ids of trajectory " + std::to_string(t.id) + " in " + file + " are not 0..n-1 in order: found " + (s_node.Find("id") ? *s_node.Find("id") : std::string("none")) +
               " at position " + std::to_string(t.submaps.size());
        return false;
      }
      static const char* const keys[6] = {"tx", "ty", "tz", "rx", "ry", "rz"};
      for (int c = 0; c < 6; ++c) if (!number(s_node, keys[c], &s.pose6[c])) return false;
      if (dx != 0.0) s.pose6[0] += dx;                                    // (an offset of zero leaves the bits, -0 included)
      if (dy != 0.0) s.pose6[1] += dy;
      s.pose = WithoutNegativeZero(Vector6ToTransform(s.pose6));
      if (const std::string* c = s_node.Find("connections")) s.connections = ConnectionsStrToIds(*c);
      if (const std::string* f = s_node.Find("file")) s.file = *f;
      s.dir = dir;
      if (s.file.empty() || !FileExist(s.Path())) { *why = "submap file does not exist: " + s.Path() + " (submap " + s.id.DebugString() + " of " + file + ")"; return false; }
      t.submaps.push_back(std::move(s));
    }
    m.trajectories.push_back(std::move(t));
  }
  for (const MapTrajectory& t : m.trajectories)
    for (const MapSubmap& s : t.submaps)
      for (const SubmapId& c : s.connections)
        if (c.trajectory_index < 0 || c.trajectory_index >= static_cast<int>(m.trajectories.size()) || c.submap_index < 0 ||
            c.submap_index >= static_cast<int>(m.trajectories[static_cast<size_t>(c.trajectory_index)].submaps.size())) {
          *why = "connection [" + std::to_string(c.trajectory_index) + "," + std::to_string(c.submap_index) + "] of submap " + s.id.DebugString() + " in " + file +
                 " names a submap that does not exist";
          return false;
        }
  *out = std::move(m);
  return true;
}

// the text SaveWholeMap writes: every trajectory with the base offset, attributes in the reference's order, numbers as %.17g
inline std::string TrajectoryMapXml(const TrajectoryMap& map) {
  auto num = [](double v) { char b[40]; std::snprintf(b, sizeof(b), "%.17g", v); return std::string(b); };
  std::string s = "<?xml version=\"1.0\"?>\n<Map>\n";
  for (const MapTrajectory& t : map.trajectories) {
    s += "\t<Trajectory id=\"" + std::to_string(t.id) + "\" enu_x=\"" + num(map.base_x) + "\" enu_y=\"" + num(map.base_y) + "\">\n";
    for (const MapSubmap& m : t.submaps) {
      s += "\t\t<Submap id=\"" + std::to_string(m.id.submap_index) + "\" file=\"" + xml::Encode(m.file) + "\"";
      static const char* const keys[6] = {"tx", "ty", "tz", "rx", "ry", "rz"};
      for (int c = 0; c < 6; ++c) s += std::string(" ") + keys[c] + "=\"" + num(m.pose6[c]) + "\"";
      s += " connections=\"" + ConnectionsIdsToStr(m.connections) + "\" />\n";
    }
    s += "\t</Trajectory>\n";
  }
  s += "</Map>\n";
  return s;
}
inline bool WriteTrajectoryMap(const std::string& file, const TrajectoryMap& map, std::string* why = nullptr) {
  std::ofstream out(file, std::ios::binary);
  out << TrajectoryMapXml(map);
  out.close();
  if (!out) { if (why) *why = "cannot write " + file; return false; }
  return true;
}

// ---- submap cloud files ------------------------------------------------------------------------------------------------------------

inline bool WriteSubmapCloud(const std::string& file, const data::InnerCloudType& cloud, std::string* why = nullptr) {
  static_assert(sizeof(data::InnerPointType) == 20 && sizeof(float) == 4, "20-byte rows");
  std::ofstream out(file, std::ios::binary);
  const uint64_t ns = cloud.stamp < 0 ? 0 : static_cast<uint64_t>(cloud.stamp);
  const uint32_t head[3] = {static_cast<uint32_t>(ns / 1000000000ull), static_cast<uint32_t>(ns % 1000000000ull), 1u};
  const uint64_t count = cloud.points.size();
  out.write(reinterpret_cast<const char*>(head), 12);
  out.write(reinterpret_cast<const char*>(&count), 8);
  if (count) out.write(reinterpret_cast<const char*>(cloud.points.data()), static_cast<std::streamsize>(20 * count));
  out.close();
  if (!out) { if (why) *why = "cannot write " + file; return false; }
  return true;
}
inline bool ReadSubmapCloud(const std::string& file, data::InnerCloudType* cloud, std::string* why = nullptr) {
  std::string sink;
  if (!why) why = &sink;
  std::ifstream in(file, std::ios::binary | std::ios::ate);
  if (!in) { *why = "submap file does not exist: " + file; return false; }
  const uint64_t bytes = static_cast<uint64_t>(in.tellg());
  in.seekg(0);
  uint32_t head[3] = {0, 0, 0};
  uint64_t count = 0;
  if (bytes < 20 || !in.read(reinterpret_cast<char*>(head), 12) || !in.read(reinterpret_cast<char*>(&count), 8)) { *why = "submap file " + file + " is shorter than its 20-byte head"; return false; }
  if (count > (bytes - 20) / 20 || 20 + 20 * count != bytes) {
    *why = "submap file " + file + " holds " + std::to_string(bytes) + " bytes, which is not 20 + 20 x its count of " + std::to_string(count);
    return false;
  }
  cloud->stamp = static_cast<int64_t>(static_cast<uint64_t>(head[0]) * 1000000000ull + head[1]);
  cloud->points.resize(static_cast<size_t>(count));
  if (count && !in.read(reinterpret_cast<char*>(cloud->points.data()), static_cast<std::streamsize>(20 * count))) { *why = "submap file " + file + " could not be read"; return false; }
  return true;
}

}  // namespace builder
}  // namespace smhip

#endif  // SMHIP_TRAJECTORY_MAP_H_
