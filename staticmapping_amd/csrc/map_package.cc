// map_package.cc -- smhip_map_package_plan: the C ABI over map_package_plan.h.  Host only: no device, no handle.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/smhip.h"
#include "map_package_plan.h"

extern "C" {

void smhip_map_package_default_options(smhip_map_package_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->border_offset = 100.0;                       // MapPackageOptions, builder/map_package.h:36-41
  o->piece_width = 500.0;
}

smhip_status smhip_map_package_plan(int n_submaps, const double* translations, const smhip_map_package_options* opts, int32_t steps[2],
                                    int piece_capacity, double* centres, double* boxes, int32_t* member_offsets, int member_capacity,
                                    int32_t* members, int32_t* n_members, char* why, int why_len) {
  auto say = [&](const std::string& text) { if (why && why_len > 0) std::snprintf(why, static_cast<size_t>(why_len), "%s", text.c_str()); };
  say("");
  if (!opts || !steps || piece_capacity < 0 || member_capacity < 0) { say("null options or step counts, or a negative capacity"); return SMHIP_ERR_INVALID_ARGUMENT; }
  smhip_map_package::Plan plan;
  std::string reason;
  if (!smhip_map_package::MakePlan(n_submaps, translations, opts->border_offset, opts->piece_width, &plan, &reason)) {
    say(reason);
    return SMHIP_ERR_INVALID_ARGUMENT;
  }
  steps[0] = plan.x_steps; steps[1] = plan.y_steps;
  if (n_members) *n_members = static_cast<int32_t>(plan.members.size());
  const size_t P = plan.pieces.size();
  if (static_cast<size_t>(piece_capacity) < P) return SMHIP_OK;            // the counting call
  for (size_t i = 0; i < P; ++i) {
    const smhip_map_package::Piece& p = plan.pieces[i];
    if (centres) { centres[2 * i] = p.centre[0]; centres[2 * i + 1] = p.centre[1]; }
    if (boxes) { boxes[4 * i] = p.bb_min[0]; boxes[4 * i + 1] = p.bb_min[1]; boxes[4 * i + 2] = p.bb_max[0]; boxes[4 * i + 3] = p.bb_max[1]; }
  }
  if (member_offsets) std::memcpy(member_offsets, plan.member_offsets.data(), sizeof(int32_t) * (P + 1));
  if (members && static_cast<size_t>(member_capacity) >= plan.members.size() && !plan.members.empty())
    std::memcpy(members, plan.members.data(), sizeof(int32_t) * plan.members.size());
  return SMHIP_OK;
}

}  // extern "C"
