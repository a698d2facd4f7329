// map_package_plan.h -- the plan of SaveTrajectoriesAsMapPackage (the reference's builder/map_package.cc:59-141): which square
// pieces the static map is cut into and which submaps each piece is built from.  Host only, doubles only, no device.
//
//   extent          min / max of the submaps' global translations in x and y, widened by border_offset (:60-86)
//   step counts     int((max - min) / half_width), truncating, half_width = piece_width * 0.5; a negative count refuses the package
//                   (:89-95), a count of 0 becomes 1 (:103-108)
//   piece (x, y)    centre = min + (x + 1) * half_width; box = centre -+ half_width, each bound clamped to [min, max] (:122-128)
//   members         the submaps whose translation lies in the box widened by border_offset, closed comparisons, in trajectory
//                   order (:110-115, 130-139)
//
// Not the reference's, decided here: refused before any work are a piece_width that is not finite and positive and a
// border_offset that is not finite (the reference would divide by zero), no submap at all and a translation that is not finite
// (its int conversion would be undefined), and a plan of more than kMaxPieces pieces (the reference puts the pieces in an array on
// the stack).
#ifndef SMHIP_MAP_PACKAGE_PLAN_H_
#define SMHIP_MAP_PACKAGE_PLAN_H_

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace smhip_map_package {

constexpr int kMaxPieces = 65536;

struct Piece { double centre[2], bb_min[2], bb_max[2]; };
struct Plan {
  int x_steps = 0, y_steps = 0;
  std::vector<Piece> pieces;                 // x-major: piece (x, y) at x * y_steps + y
  std::vector<int32_t> member_offsets;       // pieces + 1
  std::vector<int32_t> members;
};

inline double Clamp(double v, double lo, double hi) { return v > hi ? hi : (v < lo ? lo : v); }     // common::Clamp, common/math.h:66-75
inline bool InsideBbox(double px, double py, const double bb_min[2], const double bb_max[2]) {      // :110-115
  return px >= bb_min[0] && px <= bb_max[0] && py >= bb_min[1] && py <= bb_max[1];
}

// translations: n x 3 doubles (Submap::GlobalTranslation).  false: refused, the reason in *why.
inline bool MakePlan(int n, const double* translations, double border_offset, double piece_width, Plan* plan, std::string* why) {
  *plan = Plan();
  if (n < 1 || translations == nullptr) { *why = "no submaps"; return false; }
  if (!std::isfinite(piece_width) || !(piece_width > 0.0)) { *why = "piece_width must be finite and positive"; return false; }
  if (!std::isfinite(border_offset)) { *why = "border_offset must be finite"; return false; }
  double min_x = 1.e50, max_x = -1.e50, min_y = 1.e50, max_y = -1.e50;                              // :60-81
  for (int i = 0; i < n; ++i) {
    const double px = translations[3 * i], py = translations[3 * i + 1];
    if (!std::isfinite(px) || !std::isfinite(py)) { *why = "a submap's translation is not finite"; return false; }
    if (px > max_x) max_x = px;
    if (px < min_x) min_x = px;
    if (py > max_y) max_y = py;
    if (py < min_y) min_y = py;
  }
  min_x -= border_offset; min_y -= border_offset; max_x += border_offset; max_y += border_offset;   // :83-86
  const double half_width = piece_width * 0.5;                                                      // :89
  const double qx = (max_x - min_x) / half_width, qy = (max_y - min_y) / half_width;
  if (!std::isfinite(qx) || !std::isfinite(qy)) { *why = "the extent over half the piece width is not finite"; return false; }
  if (qx > kMaxPieces + 1.0 || qy > kMaxPieces + 1.0) { *why = "more than 65536 pieces"; return false; }
  if (qx <= -2147483648.0 || qy <= -2147483648.0) { *why = "No good bounding box, save no map package."; return false; }
  int x_steps = static_cast<int>(qx), y_steps = static_cast<int>(qy);                               // :90-91, truncating
  if (x_steps < 0 || y_steps < 0) { *why = "No good bounding box, save no map package."; return false; }   // :92-95
  if (x_steps == 0) x_steps++;                                                                      // :103-108
  if (y_steps == 0) y_steps++;
  if (static_cast<long long>(x_steps) * y_steps > kMaxPieces) { *why = "more than 65536 pieces"; return false; }
  plan->x_steps = x_steps; plan->y_steps = y_steps;
  plan->pieces.resize(static_cast<size_t>(x_steps) * y_steps);
  plan->member_offsets.assign(1, 0);
  for (int x = 0; x < x_steps; ++x) {
    for (int y = 0; y < y_steps; ++y) {
      Piece& p = plan->pieces[static_cast<size_t>(x) * y_steps + y];
      p.centre[0] = min_x + (x + 1) * half_width; p.centre[1] = min_y + (y + 1) * half_width;       // :122
      p.bb_min[0] = Clamp(p.centre[0] - half_width, min_x, max_x); p.bb_max[0] = Clamp(p.centre[0] + half_width, min_x, max_x);   // :123-128
      p.bb_min[1] = Clamp(p.centre[1] - half_width, min_y, max_y); p.bb_max[1] = Clamp(p.centre[1] + half_width, min_y, max_y);
      const double lo[2] = {p.bb_min[0] - border_offset, p.bb_min[1] - border_offset};              // :130-131
      const double hi[2] = {p.bb_max[0] + border_offset, p.bb_max[1] + border_offset};
      for (int i = 0; i < n; ++i)
        if (InsideBbox(translations[3 * i], translations[3 * i + 1], lo, hi)) plan->members.push_back(i);   // :132-139
      if (plan->members.size() > 0x7fffffffu) { *why = "more than 2^31 piece members"; *plan = Plan(); return false; }
      plan->member_offsets.push_back(static_cast<int32_t>(plan->members.size()));
    }
  }
  return true;
}

}  // namespace smhip_map_package
#endif  // SMHIP_MAP_PACKAGE_PLAN_H_
