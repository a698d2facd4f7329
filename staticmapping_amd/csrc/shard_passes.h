// shard_passes.h -- what rank 0 of smhip_shard does once the pose file is written: --map, --submap-edges, --close-loops and
// --map-package, each from the poses AS WRITTEN, run by RunPasses in that order.
// The three passes over submaps are loops over one SubmapFeed: the submaps of the sequence, one after the other, resident on the device.
#pragma once

#include <sys/stat.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/smhip.h"
#include "../../include/smhip/kitti_scans.h"
#include "../../include/smhip/pcd.h"
#include "../../include/smhip/back_end.h"
#include "../../include/smhip/pose_graph.h"
#include "../../include/smhip/map_package.h"
#include "../../include/smhip/multi_trajectory.h"
#include "../../include/smhip/sweep_motion.h"
#include "shard_poses.h"

namespace shard {

using smhip::kitti::kMaxFloatsPerFile;
using smhip::kitti::ScanPrefetcher;

struct Args {
  std::string scans_dir, out_path = "kitti_pose.txt", id_file;
  unsigned long long nonce = 0;             // identifies this run's id file (launcher: pid and start time; else MASTER_PORT)
  int gpus = 1, rank = -1, world = -1, local_rank = -1;
  int batch = 256, iterations = 20, early_exit = 0, max_pairs = -1, readers = 8, matchers = 1, warmup = 1, parts = 0;
  double guess_tx = 0.0;
  std::string guess = "constant";          // --guess constant|ctrv: every pair from the --guess-tx step, or pair k + 1 from pair k's result (one rank, one matcher)
  bool quiet = false;
  // the static map (--map); the MRVM settings are MrvmSettings' (multi_resolution_voxel_map.h:54-65), whose defaults these are
  std::string map_path, map_poses;
  int map_every = 1, map_part_every = 0, map_points_per_cell = 10, map_max_table_log2 = 28;
  float map_resolution = 0.1f, map_threshold = 0.6f, map_hit = 0.55f, map_miss = 0.48f, map_z_offset = 0.f;
  bool map_average = false, map_rgb = false;
  // --map-compensate 1: --map and --map-package de-skew every frame by its sweep motion, taken from the pose file (smhip/sweep_motion.h)
  bool map_compensate = false, map_compensate_given = false;
  // the map package (--map-package); defaults: MapPackageOptions, builder/map_package.h:36-41
  std::string map_package;
  smhip::MapPackageOptions package;
  // consecutive submaps (--submap-edges); defaults: builder/submap_options.h:30-38 and accepted_min_score of the configs
  std::string submap_edges;
  int submap_frames = 5;
  float submap_voxel = 0.1f, submap_min_score = 0.7f;
  // --close-loops: the pose graph over those submaps; the detector's settings (back_end/loop_detector_options.h:29-40), with the
  // descriptor gate on as in the shipped KITTI config
  std::string close_loops;
  smhip::back_end::LoopDetectorSettings loop = [] { smhip::back_end::LoopDetectorSettings s; s.use_descriptor = true; return s; }();
  // --loop-huber K: IsamOptimizerOptions::loop_closure_huber, the Huber threshold of every loop edge (0: none); --loop-report FILE: a
  // line per loop edge after the last solve
  double loop_huber = 0.0;
  bool loop_huber_given = false;
  std::string loop_report;
  // --loop-guess-search 1: LoopDetectorSettings::guess_search (in `loop` above), the correlative search around every candidate's
  // pose-derived guess before its ICP; --loop-guess-resolution R and --loop-guess-window half_xy,half_z,yaw_steps,yaw_step_deg set its
  // options.  With it on, every --loop-report line gains search_score guess_score runner_up_score search_used.
  bool loop_guess_given = false;
  // --pose-covariance FILE: after the final optimisation, every submap's marginal covariance (include/smhip.h, "Marginal covariances"):
  // a line per submap, `index held sigma_rot[3] sigma_pos_world[3] cov[21]` -- held: 1 for the submap the graph holds (all zeros);
  // sigma_rot: the square roots of the rotation part's diagonal, rad, in the submap's own frame; sigma_pos_world: those of the diagonal
  // of R Sigma_vv R^T, m; cov[21]: the upper triangle of the 6x6, row by row, %.9g -- then one line each, labelled `calib` and
  // `gps_frame` in place of the index, for the calibration and GPS-frame vertices when the graph has them.  Relative to the held submap.
  std::string pose_covariance;
  // --pose-covariance-chunk N: the nodes asked for in one marginals call (256: a workgroup then runs one query);
  // --pose-graph-dump FILE: the final optimisation's input as text, so that the solve and its covariances can be replayed from the
  // file alone: "n m", a line per node (16 numbers of the pose, column-major, then held), a line per factor (kind i j, 16 data, 6
  // sigmas, the Huber threshold, 1 and 36 numbers of the square-root information or 0), all %.17g
  int pose_covariance_chunk = 256;
  std::string pose_graph_dump;
  // --edge-information 1: every accepted consecutive-submap match and every loop edge is measured with its own 6x6 information and
  // enters the graph with it (smhip/edge_information.h); --edge-information-scale S: EdgeInformationOptions::information_scale;
  // --edge-report FILE: a line per measured edge
  bool edge_information = false, edge_information_given = false, edge_information_scale_given = false;
  double edge_information_scale = 1.0;
  std::string edge_report;
  // --gps-enu FILE: one line per scan in file order, three numbers already in ENU metres, nan = no fix (the geodetic conversion is
  // not restated); the factors' settings (isam_optimizer.h:61-66) and the antenna in the tracking frame
  std::string gps_enu;
  std::vector<std::array<double, 3>> enu;
  double gps_lever[3] = {0.0, 0.0, 0.0};
  int gps_init_num = 25, gps_sample_step = 1;
  double gps_init_angle = 1.6;
  bool gps_output_enu = false;
  // --odom FILE: one line per scan in file order, 12 numbers: the odometer's pose as a row-major 3 x 4, any nan = no reading; the
  // readings are taken relative to the first finite line (data_collector.cc:179-184).  --odom-tf tx,ty,tz,rx,ry,rz: the initial
  // odom -> lidar transform (common::Vector6ToTransform: R = Rz Ry Rx); --odom-calib: estimate it; --odom-huber K: the factors' threshold
  std::string odom_file;
  std::vector<std::array<double, 16>> odom;       // column-major 4 x 4, relative to the first reading; [15] = 0 marks "no reading"
  double odom_tf[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool odom_tf_given = false, odom_calib = false, odom_huber_given = false;
  double odom_huber = 1.0;
  // --save-trajectory-map DIR (with --close-loops): DIR/map.xml and a cloud file per submap, the files a later join loads
  std::string save_trajectory_map;
  // the join, a run of its own without --scans: --join-base A/map.xml --join-incremental B/map.xml --join-out C/map.xml
  // [--join-hold-base 1] [--join-connection-huber K] [--join-pcd whole.pcd] [--join-static-map static.pcd]; it shares --loop-* and
  // --loop-report, and --loop-huber defaults to the multi-trajectory optimiser's 1 there
  std::string join_base, join_incremental, join_out, join_pcd, join_static_map;
  bool join_hold_base = false, join_option_given = false;
  double join_connection_huber = 0.0;
  bool Join() const { return !join_base.empty() || !join_incremental.empty() || !join_out.empty(); }
};

// the file can be written, or created where it is -- decided without creating or truncating it
inline bool CanWrite(const std::string& path) {
  if (::access(path.c_str(), F_OK) == 0) return ::access(path.c_str(), W_OK) == 0;
  const size_t cut = path.find_last_of('/');
  const std::string dir = cut == std::string::npos ? "." : (cut == 0 ? "/" : path.substr(0, cut));
  return ::access(dir.c_str(), W_OK | X_OK) == 0;
}
[[noreturn]] inline void Die(const std::string& m) { std::fprintf(stderr, "smhip_shard: %s\n", m.c_str()); std::exit(2); }

inline std::string Fmt(const char* fmt, ...) {
  va_list ap, aq;
  va_start(ap, fmt);
  va_copy(aq, ap);
  const int n = std::vsnprintf(nullptr, 0, fmt, ap);
  va_end(ap);
  std::string out(static_cast<size_t>(std::max(n, 0)) + 1, '\0');
  std::vsnprintf(&out[0], out.size(), fmt, aq);
  va_end(aq);
  out.resize(static_cast<size_t>(std::max(n, 0)));
  return out;
}

inline double Since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); }

// room per read buffer for files of at most max_bytes: a row is 16 bytes, the reader stops at kMaxFloatsPerFile
inline size_t SlotFloats(size_t max_bytes) { return std::min(kMaxFloatsPerFile, (max_bytes / 16 + 1) * 4); }

// the frames --map inserts: 0, K, 2K, ... below n_frames (--map-every K stands in for the reference's key-frame selection)
inline std::vector<int> MapFrames(const Args& a, int n_frames) {
  std::vector<int> v;
  for (int k = 0; k < n_frames; k += a.map_every) v.push_back(k);
  return v;
}

// --map PATH: the static map of MapBuilder::SaveMaps (builder/map_builder.cc:825-910).  Once kitti_pose.txt is written and the matchers
// are gone, rank 0 reads the scans of `frames` again in order and inserts frame k's raw rows (intensity x 255, kitti_reader.cc:113)
// under poses[k] into one device MultiResolutionVoxelMap (ApplyTransformToOutput on the device, origin = the pose's translation).
// The poses are the ones AS WRITTEN to the pose file (8 significant digits, parsed back), so the map is a function of that file:
// --map-poses FILE builds the same map, byte for byte, with no alignment, no RCCL and one process -- also from poses that came from
// elsewhere.  --map-part-every N writes <stem>_part_<i>.pcd after every N inserted frames and starts a fresh map (separate_output /
// separate_step, :860-890, counted in frames rather than submaps); otherwise the whole map goes to PATH.  Every file is a PCD file
// with its rows in voxel-key order (SMHIP_MRVM_SORTED).  Returns 0, or 3 when the map refused a frame: the files of this run are then
// removed.  map_voxels / map_points are summed over the parts.  Like every pass, it appends its fields of the summary line when it returns 0.
// --map-compensate 1 ("Motion compensation after optimisation"): frame k is de-skewed on its way in by
// SweepMotions(poses)[k], the step from its pose to its successor's in the pose file whatever --map-every says
// (smhip_mrvm_insert_compensated_f32; poses[k] is read as the pose at the start of the sweep).
inline int BuildMap(const Args& a, const std::vector<std::string>& files, const std::vector<int>& frames, const std::vector<Pose>& poses, int device,
                    std::string* fields) {
  const auto t0 = std::chrono::steady_clock::now();
  struct { int frames = 0, parts = 0; long long voxels = 0, points = 0; } res;
  size_t max_bytes = 16;
  for (int k : frames) { struct stat sb; if (stat(files[k].c_str(), &sb) == 0) max_bytes = std::max(max_bytes, static_cast<size_t>(sb.st_size)); }
  const size_t slot_floats = SlotFloats(max_bytes);
  smhip_mrvm_settings set;
  smhip_mrvm_default_settings(&set);
  set.prob_threshold = a.map_threshold; set.high_resolution = a.map_resolution; set.hit_prob = a.map_hit; set.miss_prob = a.map_miss;
  set.z_offset = a.map_z_offset; set.max_point_num_in_cell = a.map_points_per_cell;
  const int flags = SMHIP_MRVM_SORTED | (a.map_average ? SMHIP_MRVM_AVERAGE : 0) | (a.map_rgb ? SMHIP_MRVM_RGB : 0);
  std::string stem = a.map_path;
  if (stem.size() > 4 && stem.compare(stem.size() - 4, 4, ".pcd") == 0) stem.resize(stem.size() - 4);
  std::vector<std::string> written;
  smhip_mrvm_handle h = nullptr;
  auto fresh_map = [&]() {
    if (h) smhip_mrvm_destroy(h);
    h = nullptr;
    const smhip_status st = smhip_mrvm_create(device, std::min(22, a.map_max_table_log2), static_cast<int>(slot_floats / 4), &set, &h);
    if (st != SMHIP_OK) Die(std::string("smhip_mrvm_create: ") + smhip_status_string(st) + " (is this a gfx950 GPU? there is no CPU fallback)");
    if (smhip_mrvm_set_max_table_log2(h, a.map_max_table_log2) != SMHIP_OK) Die(smhip_mrvm_last_error(h));
  };
  auto write_map = [&](const std::string& path) {     // OutputToPointCloud(threshold, filename), multi_resolution_voxel_map.cc:217-242
    int v = 0, n = 0, m = 0;
    if (smhip_mrvm_voxel_count(h, &v) != SMHIP_OK || smhip_mrvm_output_ex(h, a.map_threshold, flags, nullptr, 0, &n) != SMHIP_OK) Die(smhip_mrvm_last_error(h));
    std::vector<float> rows(4 * static_cast<size_t>(n));
    if (n > 0 && smhip_mrvm_output_ex(h, a.map_threshold, flags, rows.data(), n, &m) != SMHIP_OK) Die(smhip_mrvm_last_error(h));
    if (m != n) Die("map: output changed size between two calls");
    res.voxels += v;
    if (smhip::pcd::SaveBinary(path, n > 0 ? rows.data() : nullptr, static_cast<size_t>(n), a.map_rgb)) {
      written.push_back(path);
      res.points += n;
      ++res.parts;
    }
  };
  fresh_map();
  const std::vector<Pose> motions = a.map_compensate ? smhip::SweepMotions(poses) : std::vector<Pose>();
  ScanPrefetcher scans(files, frames, a.readers, 2 * std::max(1, a.readers) + 2, /*hold_until_release=*/false, slot_floats);
  int in_part = 0, part = 0, rc = 0;
  for (size_t i = 0; i < frames.size(); ++i) {
    int n = 0, fi = -1;
    const float* rows = scans.Next(&n, &fi);
    if (!rows || fi != frames[i]) Die("map: prefetcher out of step");
    if (n < 0) Die("cannot read " + files[fi]);
    if (n == 0) {
      std::fprintf(stderr, "smhip_shard: map: %s is empty, skipped\n", files[fi].c_str());     // InsertPointCloud: "cloud is empty.", :61-64
    } else {
      const smhip_status st = a.map_compensate ? smhip_mrvm_insert_compensated_f32(h, rows, 4, n, poses[fi].data(), motions[fi].data(), 255.f)
                                               : smhip_mrvm_insert_transformed_f32(h, rows, 4, n, poses[fi].data(), 255.f);
      if (st != SMHIP_OK) {
        std::fprintf(stderr, "smhip_shard: map: frame %d refused: %s\n", fi, smhip_mrvm_last_error(h));
        rc = 3;
        break;
      }
      if (smhip_mrvm_last_error(h)[0]) std::fprintf(stderr, "smhip_shard: map: frame %d: %s\n", fi, smhip_mrvm_last_error(h));
    }
    ++res.frames;
    if (a.map_part_every > 0 && ++in_part == a.map_part_every) {
      write_map(stem + "_part_" + std::to_string(part++) + ".pcd");
      fresh_map();
      in_part = 0;
    }
  }
  if (rc == 0) {
    if (a.map_part_every == 0) write_map(a.map_path);
    else if (in_part > 0) write_map(stem + "_part_" + std::to_string(part) + ".pcd");
  } else {
    for (const auto& f : written) std::remove(f.c_str());
  }
  smhip_mrvm_destroy(h);
  const double seconds = Since(t0);
  if (rc == 0)
    *fields += Fmt(", \"map_file\": \"%s\", \"map_frames\": %d, \"map_voxels\": %lld, \"map_points\": %lld, \"map_parts\": %d, \"map_seconds\": %.4f, "
                   "\"map_ms_per_frame\": %.3f", a.map_path.c_str(), res.frames, res.voxels, res.points, res.parts, seconds,
                   res.frames > 0 ? 1e3 * seconds / res.frames : 0.0);
  return rc;
}

// ---- the submaps of the sequence, one after the other, resident on the device ------------------------------------------------
struct PairMatch { smhip_status status = SMHIP_OK; double score = 0.0; bool accepted = false; Pose transform_to_next{}; };

// Frames [kN, (k + 1)N) form submap k < S (--submap-frames N; Submap::InsertFrame, builder/submap.cc:76-163); a trailing group that is
// not full has no cloud (submap.cc:98) and is dropped.  Build(k, local) reads the N scans and builds the submap's cloud on the device
// from the raw rows under N local poses (smhip_submap_build_f32: VoxelGrid of --submap-voxel, 0 = none).  The cloud never leaves the
// device: it is the filter output of `h`, becomes the source against the previous submap's CalculateNormals target (MatchToPrevious),
// then the target of the next (KeepAsTarget).  The local poses are the caller's: the passes do not all invert the first pose the
// same way.  `label` names the pass in messages.  Build(k, local, motions) with motions != nullptr (N times 16 doubles) de-skews
// every frame by its sweep motion first (smhip_submap_build_compensated_f32).
struct SubmapFeed {
  const Args& a;
  const std::vector<std::string>& files;
  const int N;
  const std::string label;
  float voxel = 0.f;
  smhip_handle h = nullptr;
  std::unique_ptr<ScanPrefetcher> scans;

  SubmapFeed(const Args& a, const std::vector<std::string>& files, int S, int N, int device, const char* label) : a(a), files(files), N(N), label(label) {
    // capacity: the largest submap's rows together (every scan of a group is read whole)
    long long cap = 16;
    size_t max_bytes = 16;
    for (int k = 0; k < S; ++k) {
      long long rows = 0;
      for (int f = k * N; f < (k + 1) * N; ++f) {
        struct stat sb;
        if (stat(files[f].c_str(), &sb) == 0) { rows += std::min<long long>(sb.st_size / 16, kMaxFloatsPerFile / 4); max_bytes = std::max(max_bytes, static_cast<size_t>(sb.st_size)); }
      }
      cap = std::max(cap, rows);
    }
    if (cap > 4194304) Die("a submap of " + std::to_string(cap) + " points exceeds the backend's limit of 4194304 (lower --submap-frames)");
    const smhip_status st = smhip_create(device, nullptr, 1, static_cast<int>(cap), static_cast<int>(cap), &h);
    if (st != SMHIP_OK) Die("smhip_create (" + this->label + "): " + smhip_status_string(st) + " (is this a gfx950 GPU? there is no CPU fallback)");
    // the six-decimal trip of the voxel size through the filter's text (submap.cc:148-154)
    if (a.submap_voxel > 0.f) voxel = static_cast<float>(std::atof(std::to_string(a.submap_voxel).c_str()));
    std::vector<int> order(static_cast<size_t>(S) * N);
    for (size_t i = 0; i < order.size(); ++i) order[i] = static_cast<int>(i);
    scans.reset(new ScanPrefetcher(files, order, a.readers, N + std::max(1, a.readers) + 2, /*hold_until_release=*/true, SlotFloats(max_bytes)));
  }
  ~SubmapFeed() { scans.reset(); smhip_destroy(h); }

  void SetIcpOptions() {                                                  // IcpFast under --iterations and --early-exit, for the passes that match
    smhip_icp_options o;
    smhip_icp_default_options(&o);
    o.max_iteration = a.iterations;
    o.early_exit = a.early_exit;
    if (smhip_icp_set_options(h, &o) != SMHIP_OK) Die(smhip_last_error(h));
  }

  // Submap k under local[16 * f] (column-major).  Returns its point count, or -1 when the device refused it (said on stderr).
  int Build(int k, const double* local, const double* motions = nullptr) {
    std::vector<const float*> rows(N);
    std::vector<int> n(N);
    for (int f = 0; f < N; ++f) {
      int fi = -1;
      rows[f] = scans->Next(&n[f], &fi);
      if (!rows[f] || fi != k * N + f) Die(label + ": prefetcher out of step");
      if (n[f] < 0) Die("cannot read " + files[fi]);
    }
    int m = 0;
    const smhip_status st = motions ? smhip_submap_build_compensated_f32(h, N, rows.data(), 4, n.data(), local, motions, voxel, &m)
                                    : smhip_submap_build_f32(h, N, rows.data(), 4, n.data(), local, voxel, &m);
    scans->ReleaseHeld();                                                 // the call returned: the rows have left the host buffers
    if (st == SMHIP_OK) return m;
    std::fprintf(stderr, "smhip_shard: submap %d refused: %s\n", k, smhip_last_error(h));
    return -1;
  }

  // SubmapPairMatch(source = the resident submap k, target = submap k - 1), map_builder.cc:399-446: the guess from the two first
  // frames' poses (:426-428), NormalizeRotation of the result (:434), transform_to_next = the match when its score reaches
  // --submap-min-score, else the guess (:436-444).  An align that fails (no correspondence) is an edge that keeps the guess, score 0.
  // false: the device refused the cloud as source (said on stderr).
  bool MatchToPrevious(int k, const std::vector<Pose>& poses, PairMatch* pm) {
    if (smhip_filter_output_to_source(h, 0) != SMHIP_OK) { std::fprintf(stderr, "smhip_shard: submap %d as source: %s\n", k, smhip_last_error(h)); return false; }
    const Pose guess = MulPose(AffineInverse(poses[(k - 1) * N]), poses[k * N]);
    smhip::registrator::Matrix4d T;
    smhip_icp_stats stats;
    pm->status = smhip_icp_align(h, guess.data(), T.data(), &pm->score, &stats);
    if (pm->status != SMHIP_OK) {
      std::fprintf(stderr, "smhip_shard: submaps %d -> %d: %s (%s)\n", k - 1, k, smhip_status_string(pm->status), smhip_last_error(h));
      pm->score = 0.0;
    }
    pm->accepted = pm->status == SMHIP_OK && pm->score >= a.submap_min_score;
    pm->transform_to_next = guess;
    if (pm->accepted) {
      smhip::back_end::NormalizeRotation(T);
      std::copy(T.data(), T.data() + 16, pm->transform_to_next.begin());
    }
    return true;
  }

  // the resident cloud becomes the target of the next pair (Submap::Cloud() carries normals, submap.cc:160-161)
  bool KeepAsTarget(int k) {
    int m = 0;
    if (smhip_filter_output_to_target(h, 0, &m) == SMHIP_OK) return true;
    std::fprintf(stderr, "smhip_shard: submap %d as target: %s\n", k, smhip_last_error(h));
    return false;
  }
};

// the local poses of submap k as --submap-edges and --map-package take them: first^-1 * frame, the first frame's the identity itself
// (submap.cc:83-87)
inline std::vector<double> LocalPosesAsWritten(const std::vector<Pose>& poses, int k, int N) {
  std::vector<double> local(16 * static_cast<size_t>(N));
  const Pose first_inv = AffineInverse(poses[k * N]);
  for (int f = 0; f < N; ++f) {
    const Pose lp = f == 0 ? Pose{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1} : MulPose(first_inv, poses[k * N + f]);
    std::memcpy(&local[16 * static_cast<size_t>(f)], lp.data(), sizeof(double) * 16);
  }
  return local;
}

// ---- --submap-edges -------------------------------------------------------------------------------------------------------
// --submap-edges PATH: the submaps of frames [0, n_frames) under the poses as written and the match of every pair of consecutive ones
// (MapBuilder::SubmapPairMatch), IcpFast under --iterations and --early-exit.  PATH holds one line per edge: `k k+1 accepted score`
// and the twelve numbers of transform_to_next in the pose writer's format.  Returns 0, or 3 when the device refused a submap (the
// file is then removed).
inline int BuildSubmapEdges(const Args& a, const std::vector<std::string>& files, int n_frames, const std::vector<Pose>& poses, int device, std::string* fields) {
  const auto t0 = std::chrono::steady_clock::now();
  const int N = a.submap_frames, S = n_frames / N;                        // a trailing group that is not full is dropped
  std::ofstream out(a.submap_edges);
  if (!out) Die("cannot write " + a.submap_edges);
  out.precision(8);
  int rc = 0, edges = 0, accepted = 0;
  double score_sum = 0.0;
  if (S >= 2) {
    SubmapFeed feed(a, files, S, N, device, "submaps");
    feed.SetIcpOptions();
    for (int k = 0; k < S && rc == 0; ++k) {
      PairMatch pm;
      if (feed.Build(k, LocalPosesAsWritten(poses, k, N).data()) < 0 || (k > 0 && !feed.MatchToPrevious(k, poses, &pm))) { rc = 3; break; }
      if (k > 0) {
        out << (k - 1) << " " << k << " " << (pm.accepted ? 1 : 0) << " " << pm.score << " ";
        WritePoseLine(out, pm.transform_to_next.data());
        ++edges; accepted += pm.accepted ? 1 : 0; score_sum += pm.score;
      }
      if (k + 1 < S && !feed.KeepAsTarget(k)) rc = 3;
    }
  }
  out.close();
  if (rc != 0) std::remove(a.submap_edges.c_str());
  else *fields += Fmt(", \"submap_edges_file\": \"%s\", \"submaps\": %d, \"submap_edges\": %d, \"submap_edges_accepted\": %d, \"submap_mean_score\": %.6f, "
                      "\"submap_seconds\": %.4f", a.submap_edges.c_str(), S, edges, accepted, edges > 0 ? score_sum / edges : 0.0, Since(t0));
  return rc;
}

// ---- --map-package ----------------------------------------------------------------------------------------------------------
// --map-package DIR: the map package of MapBuilder::SaveMapPackage (builder/map_builder.cc:816-823, builder/map_package.cc): the
// static map cut into overlapping square pieces, DIR/<prefix><x>_<y>.pcd centred on the piece and DIR/map_package.xml listing them
// (smhip/map_package.h).  Like --map it is a function of the pose file as written, so --map-poses FILE builds it too -- also from the
// file --close-loops wrote.  Every submap (local poses first^-1 * frame; its global pose is its first frame's) is built once on the
// device and downloaded, then smhip::SaveTrajectoriesAsMapPackage over them; the pieces' voxel maps take the --map-* settings.  The
// plan is made from the poses alone before any device work: a refused plan ends the run with 2, and so does a directory the
// description cannot be written into.  Returns 0, or 3 when the device refused a submap or an insert or a piece could not be written
// (this run's files are then removed).  --map-compensate 1: the submaps are built from frames de-skewed by SweepMotions(poses).
inline int BuildMapPackage(const Args& a, const std::vector<std::string>& files, int n_frames, const std::vector<Pose>& poses, int device, std::string* fields) {
  const auto t0 = std::chrono::steady_clock::now();
  const int N = a.submap_frames, S = n_frames / N;                        // a trailing group that is not full is dropped
  if (S < 1) Die("--map-package: " + std::to_string(n_frames) + " frames hold no full submap of " + std::to_string(N));
  {
    std::vector<std::array<double, 3>> translations(static_cast<size_t>(S));
    for (int k = 0; k < S; ++k) translations[k] = {poses[k * N][12], poses[k * N][13], poses[k * N][14]};
    smhip::MapPackagePlan plan;
    std::string why;
    if (!smhip::PlanMapPackage(translations, a.package, &plan, &why)) Die("--map-package refused: " + why);
  }
  std::string dir = a.map_package;
  if (dir.back() != '/') dir += '/';
  // the description's place is taken before any device work: a directory that is missing or cannot be written ends the run here
  if (!std::ofstream(dir + a.package.descript_filename)) Die("cannot write " + dir + a.package.descript_filename);
  std::vector<smhip::MapPackageSubmap> submaps(static_cast<size_t>(S));
  int rc = 0;
  {
    SubmapFeed feed(a, files, S, N, device, "map package");     // (gone, with its device memory, before the pieces' maps are made)
    const std::vector<Pose> motions = a.map_compensate ? smhip::SweepMotions(poses) : std::vector<Pose>();
    for (int k = 0; k < S; ++k) {
      // (a vector of Pose is 16 doubles per frame, one after the other: frames kN .. kN + N - 1 are the submap's)
      const int m = feed.Build(k, LocalPosesAsWritten(poses, k, N).data(), a.map_compensate ? motions[static_cast<size_t>(k) * N].data() : nullptr);
      if (m < 0) { rc = 3; break; }
      smhip::MapPackageSubmap& sub = submaps[static_cast<size_t>(k)];
      std::memcpy(sub.global_pose.data(), poses[k * N].data(), sizeof(double) * 16);
      sub.cloud.resize(static_cast<size_t>(m));
      if (m > 0 && smhip_filter_get_output(feed.h, &sub.cloud[0].x, nullptr, m) != SMHIP_OK) {
        std::fprintf(stderr, "smhip_shard: cloud of submap %d: %s\n", k, smhip_last_error(feed.h)); rc = 3; break;
      }
    }
  }
  smhip::MapPackageResult pr;
  if (rc == 0) {
    smhip::MrvmSettings set;
    set.output_average = a.map_average; set.output_rgb = a.map_rgb; set.prob_threshold = a.map_threshold; set.high_resolution = a.map_resolution;
    set.hit_prob = a.map_hit; set.miss_prob = a.map_miss; set.z_offset = a.map_z_offset; set.max_point_num_in_cell = a.map_points_per_cell;
    // raw KITTI rows: intensity x 255 on the way into the map, as --map inserts them (kitti_reader.cc:113)
    if (!smhip::SaveTrajectoriesAsMapPackage(submaps, a.package, set, dir, &pr, device, 255.f, a.map_max_table_log2)) rc = 3;
  } else {
    std::remove((dir + a.package.descript_filename).c_str());
  }
  if (rc == 0)
    *fields += Fmt(", \"package_dir\": \"%s\", \"package_pieces\": %d, \"package_submaps\": %d, \"package_points\": %lld, \"package_seconds\": %.4f",
                   a.map_package.c_str(), pr.pieces, pr.submaps, pr.points, Since(t0));
  return rc;
}

// ---- --close-loops ------------------------------------------------------------------------------------------------------------
// --close-loops PATH: the pose graph over those submaps, MapBuilder::ConnectAllSubmap (builder/map_builder.cc:448-613), from the poses
// as written: every submap is built on the device, described where it lies (M2DP), matched against the previous one (the odometry
// factor) and handed to back_end::IsamOptimizer (smhip/pose_graph.h) -- the loop detector with the --loop-* settings
// (back_end/loop_detector_options.h:29-40), the factors, one device solve of the pose graph per update, every submap's pose written
// back.  A submap enters at the previous submap's corrected pose times its odometry factor.  After RunFinalOptimazation the frames
// get submap pose x local pose (Submap::UpdateInnerFramePose) and go to PATH in the pose writer's format, one line per frame of the
// sequence (the frames of a trailing group that is not full ride on the last submap), so --map --map-poses PATH builds the corrected
// map.  Without the flag nothing of this runs and every output is what it was.
// With --gps-enu FILE (one line per scan in file order: east north up in metres, nan = no fix; the geodetic conversion is not
// restated) a submap carries the fix of its first frame and IsamOptimizer adds the GPS / ENU factors of isam_optimizer.cc:238-349
// (--gps-lever x,y,z: the antenna in the tracking frame; --gps-init-num, --gps-sample-step, --gps-init-angle: isam_optimizer.h:61-66);
// --gps-output-enu premultiplies every submap pose by GetGpsCoordTransform() before UpdateInnerFramePose (map_builder.cc:748-762),
// so PATH is in the ENU frame.  --gps-enu without --close-loops, or a FILE whose line count is not the scan count, ends the run
// with exit 2 before any device work.
// --loop-huber K gives every loop edge, and nothing else, the Huber threshold K (IsamOptimizerOptions::loop_closure_huber; DESIGN.md
// section 6, "Robust factors"): a wrong match that settles metres off is then down-weighted instead of dragging the ring, and the JSON
// line gains "loop_edges_downweighted", the loop edges that end with a weight below 1.  --loop-report FILE writes one line per loop
// edge after the last solve, in the order added: target source norm weight (%.8g; weight 1 = taken at full weight, also without
// --loop-huber, where the norm alone shows the strain).  Either without --close-loops, or a K that is negative or not finite, ends
// the run with exit 2 before any device work.
// With --odom FILE (one line per scan in file order: 12 numbers, the odometer's pose as a row-major 3 x 4, any nan = no reading, taken
// relative to the first finite line) a submap carries the reading of its first frame and IsamOptimizer adds the odometry calibration
// factors of isam_optimizer.cc:209-224 ("Odometry calibration factor"; the model assumes that the first submap
// stands at the identity, as the pose writer's first pose does): --odom-tf tx,ty,tz,rx,ry,rz is the initial odom -> lidar transform in
// common::Vector6ToTransform's convention (default: the identity), --odom-calib frees the calibration under the reference's prior,
// --odom-huber K is the factors' threshold (default 1).  The JSON line gains "odom_factors" and "odom_tf" (the transform after the
// final solve, row-major).  --odom without --close-loops, a FILE whose line count is not the scan count or with a line that does not
// hold 12 numbers, a bad --odom-tf or K: exit 2 before any device work.
// --edge-information 1 weighs the scan-match edges by their own geometry ("Edge information"): an accepted match
// against the previous submap is measured at its result (smhip_icp_information_at on the pair as it lies on the device, with the
// matcher's dist_outlier_ratio) and handed to IsamOptimizer with AddFrame's third argument; the detector measures every loop edge it
// accepts (LoopDetectorSettings::edge_information); IsamOptimizerOptions::use_edge_information is on.  A match that was not accepted
// (the edge is the guess) or that has no information keeps the fixed sigmas.  --edge-information-scale S (finite, > 0; default 1) is
// EdgeInformationOptions::information_scale of both.  --edge-report FILE writes one line per edge that entered the graph with an
// information, chain edges first, each group in the order added: i j chain|loop kept residual_sigma, the six strengths (ascending),
// the six components of the weakest direction (rotation first; %.8g) -- the strengths are what a scale is chosen from.  The JSON line
// gains "edge_informations".  The scale or the report without --edge-information 1, or any of the three without --close-loops: exit 2
// before any device work.  Without the flag nothing of this runs and every output is what it was.
// --save-trajectory-map DIR writes, beside all this, the map a later join loads (smhip/trajectory_map.h): DIR/submap_<k>.bin, the cloud
// of submap k as it was built and matched, read back from the device, and after the final solve DIR/map.xml: one trajectory, the
// corrected submap poses, and per submap the connections to the next submap and to the source of every accepted loop edge.  Every
// other output is what it is without the flag.
// Returns 0, or 3 when the device refused something (the file is then removed and no report written).
inline std::string TrajectoryMapCloudName(int k) { return "submap_" + std::to_string(k) + ".bin"; }

inline int CloseLoops(const Args& a, const std::vector<std::string>& files, int n_frames, const std::vector<Pose>& poses, int device, std::string* fields) {
  namespace be = smhip::back_end;
  namespace bld = smhip::builder;
  using smhip::registrator::Matrix4d;
  const auto t0 = std::chrono::steady_clock::now();
  const int N = a.submap_frames, S = n_frames / N;
  struct {
    int loop_edges = 0, solves = 0, stop_reason = 0; double final_cost = 0.0, moved_m = 0.0;
    int gps_factors = 0; double gps_coord[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};    // with --gps-enu; row-major
    int downweighted = 0;                                                                             // with --loop-huber
    int odom_factors = 0; double odom_tf[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};     // with --odom; row-major
    int edge_informations = 0;                                                                        // with --edge-information
  } res;
  struct EdgeReportRow { int i, j; bool loop; be::EdgeInformation information; };
  std::vector<EdgeReportRow> edge_report;
  std::vector<smhip::back_end::LoopEdgeWeight> loop_report;
  std::vector<smhip::back_end::IsamOptimizer::LoopEdgeSearch> loop_searches;
  std::ofstream out(a.close_loops);
  if (!out) Die("cannot write " + a.close_loops);
  out.precision(8);
  std::ofstream cov_out;
  if (!a.pose_covariance.empty()) {
    cov_out.open(a.pose_covariance);
    if (!cov_out) Die("cannot write " + a.pose_covariance);
  }
  std::string cov_lines;
  double odom_tf_sigmas[6] = {0, 0, 0, 0, 0, 0};
  bool have_odom_tf_sigmas = false;
  std::string graph_dump_text;
  if (!a.save_trajectory_map.empty()) {
    struct stat sb;
    if (::mkdir(a.save_trajectory_map.c_str(), 0777) != 0 && !(::stat(a.save_trajectory_map.c_str(), &sb) == 0 && S_ISDIR(sb.st_mode))) Die("cannot create " + a.save_trajectory_map);
  }
  int rc = 0;
  if (S < 1) {
    for (int f = 0; f < n_frames; ++f) WritePoseLine(out, poses[f].data());
  } else {
    SubmapFeed feed(a, files, S, N, device, "loop closing");
    feed.SetIcpOptions();
    const smhip_handle h = feed.h;
    smhip_m2dp_options mo;
    smhip_m2dp_default_options(&mo);
    const int dlen = smhip_m2dp_length(&mo);
    be::LoopDetectorSettings settings = a.loop;
    settings.device = device;
    settings.edge_information = a.edge_information;
    settings.edge_information_options.information_scale = a.edge_information_scale;
    be::IsamOptimizerOptions io;
    io.use_gps = !a.gps_enu.empty();
    io.gps_factor_init_num = a.gps_init_num; io.gps_factor_sample_step = a.gps_sample_step; io.gps_factor_init_angle_rad = a.gps_init_angle;
    io.loop_closure_huber = a.loop_huber;
    io.use_odom = !a.odom_file.empty(); io.odom_extrinsic_calib = a.odom_calib; io.odom_huber = a.odom_huber;
    io.use_edge_information = a.edge_information;
    be::IsamOptimizer optimizer(io, settings, h);
    if (io.use_odom) optimizer.SetTransformOdomToLidar(bld::Vector6ToTransform(a.odom_tf));   // common::Vector6ToTransform: R = Rz(rz) Ry(ry) Rx(rx)
    {
      Matrix4d tracking_to_gps = Matrix4d::Identity();
      for (int c = 0; c < 3; ++c) tracking_to_gps(c, 3) = a.gps_lever[c];
      optimizer.SetTransformTrackingToGps(tracking_to_gps);
    }
    std::vector<std::shared_ptr<bld::Submap>> maps;
    std::vector<std::shared_ptr<be::LoopFrame>> frames;
    bld::SubmapOptions so;
    so.frame_count = N;
    const smhip::data::InnerCloudType::Ptr no_points(new smhip::data::InnerCloudType);   // the Submap objects keep the poses' books only
    for (int k = 0; k < S && rc == 0; ++k) {
      std::vector<double> local(16 * static_cast<size_t>(N));
      maps.emplace_back(new bld::Submap(so));
      for (int f = 0; f < N; ++f) {
        Matrix4d P;
        std::memcpy(P.data(), poses[k * N + f].data(), sizeof(double) * 16);
        maps.back()->InsertFrame(no_points, P);
        std::memcpy(&local[16 * static_cast<size_t>(f)], maps.back()->LocalPose(f).data(), sizeof(double) * 16);   // submap.cc:83-87
      }
      const int m = feed.Build(k, local.data());
      if (m < 0) { rc = 3; break; }
      std::shared_ptr<be::LoopFrame> frame(new be::LoopFrame);
      frame->descriptor.resize(static_cast<size_t>(dlen));
      if (smhip_m2dp_from_filter_output(h, &mo, frame->descriptor.data(), dlen) != SMHIP_OK) {
        std::fprintf(stderr, "smhip_shard: descriptor of submap %d: %s\n", k, smhip_last_error(h)); rc = 3; break;
      }
      {   // the cloud CloseLoop matches (Submap::Cloud(): normals calculated, submap.cc:160-161)
        std::vector<smhip::data::InnerPointType> pts(static_cast<size_t>(m));
        if (smhip_filter_get_output(h, &pts[0].x, nullptr, m) != SMHIP_OK) { std::fprintf(stderr, "smhip_shard: cloud of submap %d: %s\n", k, smhip_last_error(h)); rc = 3; break; }
        frame->cloud.reset(new smhip::data::InnerPointCloudData(pts));
        frame->cloud->CalculateNormals();
        if (!a.save_trajectory_map.empty()) {                              // the submap's cloud as the join will load it
          smhip::data::InnerCloudType cloud;
          cloud.points = pts;
          std::string why;
          if (!bld::WriteSubmapCloud(a.save_trajectory_map + "/" + TrajectoryMapCloudName(k), cloud, &why)) Die(why);
        }
      }
      Matrix4d from_last = Matrix4d::Identity();
      be::EdgeInformation chain_information;
      bool has_chain_information = false;
      if (k > 0) {
        PairMatch pm;
        if (!feed.MatchToPrevious(k, poses, &pm)) { rc = 3; break; }
        std::memcpy(from_last.data(), pm.transform_to_next.data(), sizeof(double) * 16);
        if (a.edge_information && pm.accepted) {                           // the pair is still on the device: measure it at its result
          smhip_icp_options o;
          smhip_icp_default_options(&o);                                   // SetIcpOptions leaves the matcher's dist_outlier_ratio at its default
          smhip_icp_information info;
          if (smhip_icp_information_at(h, 0, pm.transform_to_next.data(), o.dist_outlier_ratio, &info) != SMHIP_OK) {
            std::fprintf(stderr, "smhip_shard: information of submaps %d -> %d: %s\n", k - 1, k, smhip_last_error(h)); rc = 3; break;
          }
          if (info.status == SMHIP_OK) {
            be::EdgeInformationOptions eo;
            eo.information_scale = a.edge_information_scale;
            chain_information = be::MakeEdgeInformation(be::FromAbi(info), eo);
            has_chain_information = true;
            edge_report.push_back({k - 1, k, false, chain_information});
          }
        }
        frame->global_pose = be::Multiply(frames.back()->global_pose, from_last);
      } else {
        frame->global_pose = maps[0]->GlobalPose();
      }
      if (k + 1 < S && !feed.KeepAsTarget(k)) { rc = 3; break; }
      if (io.use_gps) {   // the fix of the submap's first frame, the frame whose pose is its global pose
        const std::array<double, 3>& e = a.enu[static_cast<size_t>(k) * N];
        if (std::isfinite(e[0]) && std::isfinite(e[1]) && std::isfinite(e[2])) {
          maps.back()->SetRelatedGpsInENU(e[0], e[1], e[2]);
          frame->has_enu = true;
          for (int c = 0; c < 3; ++c) frame->enu[c] = maps.back()->GetRelatedGpsInENU()[c];
        }
      }
      if (io.use_odom) {  // the reading of the submap's first frame
        const std::array<double, 16>& z = a.odom[static_cast<size_t>(k) * N];
        if (z[15] != 0.0) { frame->has_odom = true; std::memcpy(frame->odom.data(), z.data(), sizeof(double) * 16); }
      }
      frames.push_back(frame);
      if (!(has_chain_information ? optimizer.AddFrame(frame, from_last, &chain_information) : optimizer.AddFrame(frame, from_last))) { std::fprintf(stderr, "smhip_shard: the pose graph could not be optimised at submap %d\n", k); rc = 3; break; }
    }
    std::string& graph_dump = graph_dump_text;
    if (rc == 0 && !a.pose_graph_dump.empty()) {                          // the graph as the final optimisation is about to be given it
      const be::PoseGraph& g = optimizer.Graph();
      std::vector<double> gp, gd, gs, gh, gl;
      std::vector<int32_t> gij, gi;
      std::vector<uint8_t> gf, gk;
      g.FlattenFactors(&gp, &gf, &gk, &gij, &gd, &gs);
      g.FlattenHuber(&gh);
      g.FlattenInformation(&gi, &gl);
      graph_dump = Fmt("%d %d\n", g.NodeCount(), static_cast<int>(gk.size()));
      for (int k = 0; k < g.NodeCount(); ++k) {
        for (int q = 0; q < 16; ++q) graph_dump += Fmt("%.17g ", gp[16 * static_cast<size_t>(k) + q]);
        graph_dump += Fmt("%d\n", static_cast<int>(gf[static_cast<size_t>(k)]));
      }
      for (size_t f = 0; f < gk.size(); ++f) {
        graph_dump += Fmt("%d %d %d", static_cast<int>(gk[f]), gij[2 * f], gij[2 * f + 1]);
        for (int q = 0; q < 16; ++q) graph_dump += Fmt(" %.17g", gd[16 * f + q]);
        for (int q = 0; q < 6; ++q) graph_dump += Fmt(" %.17g", gs[6 * f + q]);
        graph_dump += Fmt(" %.17g %d", gh[f], gi[f] >= 0 ? 1 : 0);
        for (int q = 0; gi[f] >= 0 && q < 36; ++q) graph_dump += Fmt(" %.17g", gl[36 * static_cast<size_t>(gi[f]) + q]);
        graph_dump += "\n";
      }
    }
    if (rc == 0 && !optimizer.RunFinalOptimazation()) rc = 3;
    if (rc == 0 && (a.loop_huber > 0.0 || !a.loop_report.empty())) {
      loop_report = optimizer.LoopEdgeReport();
      if (static_cast<int>(loop_report.size()) != optimizer.LoopEdgeCount()) { std::fprintf(stderr, "smhip_shard: the loop edges' report was refused\n"); rc = 3; }
      for (const be::LoopEdgeWeight& w : loop_report) res.downweighted += w.weight < 1.0;
      loop_searches = optimizer.LoopEdgeSearches();
    }
    if (rc == 0 && (!a.pose_covariance.empty() || (io.use_odom && a.odom_calib))) {
      // the submaps (with the flag), then the calibration and GPS-frame vertices; 256 nodes a call, so that a workgroup runs one query
      const be::PoseGraph& graph = optimizer.Graph();
      std::vector<int> nodes;
      std::vector<std::string> labels;
      if (!a.pose_covariance.empty()) for (int k = 0; k < graph.VertexCount(); ++k) { nodes.push_back(k); labels.push_back(std::to_string(k)); }
      if (graph.HasCalibVertex()) { nodes.push_back(graph.CalibNodeIndex()); labels.push_back("calib"); }
      if (graph.HasFrameVertex() && !a.pose_covariance.empty()) { nodes.push_back(graph.FrameNodeIndex()); labels.push_back("gps_frame"); }
      std::vector<std::array<double, 36>> cov;
      const size_t chunk = static_cast<size_t>(a.pose_covariance_chunk);
      bool refused = false;
      for (size_t at = 0; at < nodes.size() && !refused; at += chunk) {
        const std::vector<int> part(nodes.begin() + static_cast<std::ptrdiff_t>(at), nodes.begin() + static_cast<std::ptrdiff_t>(std::min(at + chunk, nodes.size())));
        std::vector<std::array<double, 36>> got;
        if (!optimizer.MarginalCovariances(part, &got)) { refused = true; break; }
        cov.insert(cov.end(), got.begin(), got.end());
      }
      if (refused && !a.pose_covariance.empty()) { std::fprintf(stderr, "smhip_shard: the marginal covariances were refused\n"); rc = 3; }
      // (without --pose-covariance only the extrinsic's sigmas on stdout were wanted: an error bar that could not be had does not
      // cost the run its poses -- the field is left out)
      if (refused && a.pose_covariance.empty()) std::fprintf(stderr, "smhip_shard: warning: the extrinsic's covariance was refused; odom_tf_sigmas is left out\n");
      for (size_t q = 0; q < nodes.size() && rc == 0 && !refused; ++q) {
        const std::array<double, 36>& c = cov[q];
        if (nodes[q] == graph.CalibNodeIndex()) { have_odom_tf_sigmas = true; for (int d = 0; d < 6; ++d) odom_tf_sigmas[d] = std::sqrt(c[static_cast<size_t>(7 * d)]); }
        if (a.pose_covariance.empty()) continue;
        const bool held = nodes[q] < graph.VertexCount() ? graph.Fixed()[static_cast<size_t>(nodes[q])] != 0 : (nodes[q] == graph.CalibNodeIndex() && graph.CalibVertexHeld());
        const std::array<double, 9> world = graph.WorldPositionCovariance(nodes[q], c);
        cov_lines += labels[q] + Fmt(" %d", held ? 1 : 0);
        for (int d = 0; d < 3; ++d) cov_lines += Fmt(" %.9g", std::sqrt(c[static_cast<size_t>(7 * d)]));
        for (int d = 0; d < 3; ++d) cov_lines += Fmt(" %.9g", std::sqrt(world[static_cast<size_t>(4 * d)]));
        for (int r = 0; r < 6; ++r) for (int s = r; s < 6; ++s) cov_lines += Fmt(" %.9g", c[static_cast<size_t>(6 * r + s)]);
        cov_lines += "\n";
      }
    }
    if (rc == 0 && a.edge_information) {
      for (const be::LoopEdge& e : optimizer.LoopEdgesWithInformation()) edge_report.push_back({e.close_pair_index.first, e.close_pair_index.second, true, e.information});
      res.edge_informations = static_cast<int>(edge_report.size());
    }
    if (rc == 0) {
      res.loop_edges = optimizer.LoopEdgeCount(); res.solves = optimizer.SolveCount();
      res.stop_reason = optimizer.LastStats().stop_reason; res.final_cost = optimizer.LastStats().final_cost;
      // MapBuilder::CalculateCoordTransformToGps (map_builder.cc:748-762): with --gps-output-enu every submap pose is premultiplied
      // by the map origin's pose in the GPS frame before UpdateInnerFramePose, and the file is in the ENU frame
      const Matrix4d to_enu = optimizer.GetGpsCoordTransform();
      res.gps_factors = optimizer.GpsFactorCount();
      res.odom_factors = optimizer.OdomFactorCount();
      for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) res.odom_tf[4 * r + c] = optimizer.GetTransformOdomToLidar()(r, c);
      for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) res.gps_coord[4 * r + c] = to_enu(r, c);
      for (int k = 0; k < S; ++k) {
        maps[k]->SetGlobalPose(frames[k]->global_pose);
        maps[k]->UpdateInnerFramePose();                                   // map_builder.cc:598-601
        for (int f = 0; f < N; ++f) {
          const Matrix4d& G = maps[k]->FrameGlobalPose(f);
          const Pose& was = poses[k * N + f];
          res.moved_m = std::max(res.moved_m, std::sqrt((G(0, 3) - was[12]) * (G(0, 3) - was[12]) + (G(1, 3) - was[13]) * (G(1, 3) - was[13]) +
                                                          (G(2, 3) - was[14]) * (G(2, 3) - was[14])));
          if (!a.gps_output_enu) WritePoseLine(out, G.data());
        }
        if (a.gps_output_enu) {
          maps[k]->SetGlobalPose(be::Multiply(to_enu, frames[k]->global_pose));
          maps[k]->UpdateInnerFramePose();
          for (int f = 0; f < N; ++f) WritePoseLine(out, maps[k]->FrameGlobalPose(f).data());
        }
      }
      if (!a.save_trajectory_map.empty()) {
        // one trajectory at the corrected poses; a submap's connections are the next submap and the source of every loop edge it is the
        // target of (isam_optimizer.cc:136, 168), which is what GetWholeGraph lists for a vertex
        bld::TrajectoryMap map;
        map.trajectories.emplace_back();
        const std::vector<be::GraphItem> graph = optimizer.GetWholeGraph();
        for (int k = 0; k < S; ++k) {
          bld::MapSubmap s;
          s.id.submap_index = k;
          s.file = TrajectoryMapCloudName(k);
          s.SetPose(frames[k]->global_pose);
          for (const auto& c : graph[static_cast<size_t>(k)].connections) { bld::SubmapId id; id.submap_index = c.first; s.connections.push_back(id); }
          map.trajectories[0].submaps.push_back(s);
        }
        std::string why;
        if (!bld::WriteTrajectoryMap(a.save_trajectory_map + "/map.xml", map, &why)) Die(why);
      }
      Pose last;
      std::memcpy(last.data(), (a.gps_output_enu ? be::Multiply(to_enu, frames.back()->global_pose) : frames.back()->global_pose).data(), sizeof(double) * 16);
      const Pose carry = MulPose(last, AffineInverse(poses[(S - 1) * N]));
      for (int f = S * N; f < n_frames; ++f) WritePoseLine(out, MulPose(carry, poses[f]).data());
    }
  }
  out.close();
  if (rc != 0) {
    std::remove(a.close_loops.c_str());
    if (!a.pose_covariance.empty()) { cov_out.close(); std::remove(a.pose_covariance.c_str()); }
    return rc;
  }
  if (!a.pose_covariance.empty()) { cov_out << cov_lines; cov_out.close(); }
  if (!a.pose_graph_dump.empty()) {
    std::ofstream dump(a.pose_graph_dump);
    if (!dump) Die("cannot write " + a.pose_graph_dump);
    dump << graph_dump_text;
  }
  if (!a.loop_report.empty()) {
    std::ofstream rep(a.loop_report);
    if (!rep) Die("cannot write " + a.loop_report);
    for (size_t e = 0; e < loop_report.size(); ++e) {
      const smhip::back_end::LoopEdgeWeight& w = loop_report[e];
      rep << Fmt("%d %d %.8g %.8g", w.target, w.source, w.norm, w.weight);
      if (a.loop.guess_search && e < loop_searches.size())
        rep << Fmt(" %d %d %d %d", loop_searches[e].search_score, loop_searches[e].guess_score, loop_searches[e].runner_up_score, loop_searches[e].search_used ? 1 : 0);
      rep << "\n";
    }
  }
  if (!a.edge_report.empty()) {
    std::ofstream rep(a.edge_report);
    if (!rep) Die("cannot write " + a.edge_report);
    for (const EdgeReportRow& e : edge_report) {
      rep << Fmt("%d %d %s %d %.8g", e.i, e.j, e.loop ? "loop" : "chain", e.information.kept, e.information.residual_sigma);
      for (double v : e.information.strength) rep << Fmt(" %.8g", v);
      for (double v : e.information.weakest) rep << Fmt(" %.8g", v);
      rep << "\n";
    }
  }
  *fields += Fmt(", \"close_loops_file\": \"%s\", \"loop_submaps\": %d, \"loop_edges\": %d, \"pose_graph_solves\": %d, \"pose_graph_stop_reason\": %d, "
                 "\"pose_graph_final_cost\": %.6g, \"loop_largest_correction_m\": %.4f, \"close_loops_seconds\": %.4f", a.close_loops.c_str(), S,
                 res.loop_edges, res.solves, res.stop_reason, res.final_cost, res.moved_m, Since(t0));
  if (a.loop_huber > 0.0) *fields += Fmt(", \"loop_edges_downweighted\": %d", res.downweighted);
  if (a.edge_information) *fields += Fmt(", \"edge_informations\": %d", res.edge_informations);
  if (!a.gps_enu.empty()) {
    *fields += Fmt(", \"gps_factors\": %d, \"gps_coord\": [", res.gps_factors);
    for (int q = 0; q < 16; ++q) *fields += Fmt("%.17g%s", res.gps_coord[q], q == 15 ? "]" : ", ");
  }
  if (!a.odom_file.empty()) {
    *fields += Fmt(", \"odom_factors\": %d, \"odom_tf\": [", res.odom_factors);
    for (int q = 0; q < 16; ++q) *fields += Fmt("%.17g%s", res.odom_tf[q], q == 15 ? "]" : ", ");
    if (a.odom_calib && have_odom_tf_sigmas) {   // of the calibration vertex (lidar -> odom, the inverse of odom_tf) in its own tangent chart: rad x 3, m x 3
      *fields += ", \"odom_tf_sigmas\": [";
      for (int d = 0; d < 6; ++d) *fields += Fmt("%.9g%s", odom_tf_sigmas[d], d == 5 ? "]" : ", ");
    }
  }
  if (!a.pose_covariance.empty()) *fields += Fmt(", \"pose_covariance_file\": \"%s\"", a.pose_covariance.c_str());
  return 0;
}

// ---- the join -----------------------------------------------------------------------------------------------------------------
// --join-base A/map.xml --join-incremental B/map.xml --join-out C/map.xml: MultiTrajectoryMapBuilder (smhip/multi_trajectory.h) end to
// end, a run of its own without --scans.  Both files are read and checked before any device work (exit 2 with the reader's reason);
// then the base map's submaps enter the graph, the incremental map's with loop detection against the base (the --loop-* settings;
// --loop-huber defaults to 1 here), one solve, and the joined map goes to --join-out.  A submap file beside --join-out keeps its name
// there, any other is named by its full path.  --join-hold-base 1 holds the base map's poses; --join-connection-huber K puts the
// threshold K on the connections (the reference's 1; default 0); --join-pcd and --join-static-map write the whole map and the static
// map; --loop-report a line per cross edge (nodes in the joined order).  Returns 0, or 3 when the device refused something.
inline int JoinMaps(const Args& a, int device) {
  namespace bld = smhip::builder;
  const auto t0 = std::chrono::steady_clock::now();
  long long cap = 1 << 16;
  for (const std::string* file : {&a.join_base, &a.join_incremental}) {
    bld::TrajectoryMap m;
    std::string why;
    if (!bld::ReadTrajectoryMap(*file, &m, &why)) Die(why);
    if (m.SubmapCount() == 0) Die(*file + " holds no submap");
    for (const bld::MapTrajectory& t : m.trajectories)
      for (const bld::MapSubmap& s : t.submaps) { struct stat sb; if (::stat(s.Path().c_str(), &sb) == 0) cap = std::max<long long>(cap, (sb.st_size - 20) / 20); }
  }
  if (cap > 4194304) Die("a submap of " + std::to_string(cap) + " points exceeds the backend's limit of 4194304");
  smhip_handle h = nullptr;
  const smhip_status st = smhip_create(device, nullptr, 1, static_cast<int>(cap), static_cast<int>(cap), &h);
  if (st != SMHIP_OK) Die(std::string("smhip_create (join): ") + smhip_status_string(st) + " (is this a gfx950 GPU? there is no CPU fallback)");
  int rc = 0;
  std::string line;
  {
    smhip::MultiTrajectoryMapBuilderOptions o;
    o.loop_detect_settings = a.loop;
    o.loop_detect_settings.device = device;
    o.loop_detect_settings.max_points = static_cast<int>(cap);
    o.optimizer.hold_base_map = a.join_hold_base;
    o.optimizer.connection_huber = a.join_connection_huber;
    o.optimizer.loop_closure_huber = a.loop_huber_given ? a.loop_huber : 1.0;
    o.device = device;
    smhip::MultiTrajectoryMapBuilder builder(o, h, cap);
    auto failed = [&](const char* what) { std::fprintf(stderr, "smhip_shard: join: %s: %s\n", what, builder.LastError().c_str()); rc = 3; };
    if (!builder.LoadBaseMap(a.join_base)) failed("base map");
    if (rc == 0 && !builder.LoadIncrementalMap(a.join_incremental)) failed("incremental map");
    if (rc == 0 && !builder.SaveWholeMap(a.join_out)) failed("joined map");
    std::vector<smhip::back_end::LoopEdgeWeight> report;
    if (rc == 0) {
      report = builder.Optimizer()->LoopEdgeReport();
      if (static_cast<int>(report.size()) != builder.Optimizer()->LoopEdgeCount()) { std::fprintf(stderr, "smhip_shard: join: the cross edges' report was refused\n"); rc = 3; }
    }
    if (rc == 0 && !a.loop_report.empty()) {
      std::ofstream rep(a.loop_report);
      if (!rep) Die("cannot write " + a.loop_report);
      for (const smhip::back_end::LoopEdgeWeight& w : report) rep << Fmt("%d %d %.8g %.8g\n", w.target, w.source, w.norm, w.weight);
    }
    if (rc == 0 && !a.join_pcd.empty() && !builder.GenerateWholeMapPcd(a.join_pcd)) failed("whole-map PCD");
    if (rc == 0 && !a.join_static_map.empty() && !builder.GenerateStaticMap(a.join_static_map)) failed("static map");
    if (rc == 0) {
      const smhip_pose_graph_stats& stats = builder.Optimizer()->LastStats();
      int down = 0;
      for (const smhip::back_end::LoopEdgeWeight& w : report) down += w.weight < 1.0;
      line = Fmt("{\"driver\": \"smhip_shard (join)\", \"join_base\": \"%s\", \"join_incremental\": \"%s\", \"join_out\": \"%s\", \"join_hold_base\": %d, "
                 "\"join_base_submaps\": %d, \"join_incremental_submaps\": %d, \"join_loop_edges\": %d, \"join_loop_edges_downweighted\": %d, "
                 "\"join_pose_graph_stop_reason\": %d, \"join_pose_graph_final_cost\": %.6g, \"join_pcg_iterations\": %d, \"join_solve_seconds\": %.4f",
                 a.join_base.c_str(), a.join_incremental.c_str(), a.join_out.c_str(), a.join_hold_base ? 1 : 0, builder.BaseSubmapCount(), builder.IncrementalSubmapCount(),
                 builder.Optimizer()->LoopEdgeCount(), down, stats.stop_reason, stats.final_cost, stats.pcg_iterations, builder.SolveSeconds());
      if (!a.join_pcd.empty()) line += Fmt(", \"join_pcd\": \"%s\", \"join_pcd_points\": %lld", a.join_pcd.c_str(), builder.WholeMapPoints());
      if (!a.join_static_map.empty()) line += Fmt(", \"join_static_map\": \"%s\", \"join_static_map_voxels\": %d", a.join_static_map.c_str(), builder.StaticMapVoxels());
      line += Fmt(", \"join_seconds\": %.4f}", Since(t0));
    }
  }
  smhip_destroy(h);
  if (rc == 0 && !a.quiet) std::printf("%s\n", line.c_str());
  return rc;
}

// ---- the passes, in their order ----------------------------------------------------------------------------------------------
inline bool AnyPass(const Args& a) { return !a.map_path.empty() || !a.submap_edges.empty() || !a.close_loops.empty() || !a.map_package.empty(); }

// map, submap edges, close loops, map package: each when its flag is set, from frames [0, n_frames) under `poses`; stops at the
// first pass that fails and returns its status.  Every pass that returns 0 has appended its fields of the summary line.
inline int RunPasses(const Args& a, const std::vector<std::string>& files, int n_frames, const std::vector<Pose>& poses, int device, std::string* fields) {
  int rc = 0;
  if (rc == 0 && !a.map_path.empty()) rc = BuildMap(a, files, MapFrames(a, n_frames), poses, device, fields);
  if (rc == 0 && !a.submap_edges.empty()) rc = BuildSubmapEdges(a, files, n_frames, poses, device, fields);
  if (rc == 0 && !a.close_loops.empty()) rc = CloseLoops(a, files, n_frames, poses, device, fields);
  if (rc == 0 && !a.map_package.empty()) rc = BuildMapPackage(a, files, n_frames, poses, device, fields);
  if (rc == 0 && a.map_compensate) *fields += ", \"map_compensated\": 1";
  return rc;
}

}  // namespace shard
