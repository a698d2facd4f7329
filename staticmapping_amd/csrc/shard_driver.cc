// shard_driver.cc -- BASELINE config #4 as a C++ program: scan-to-scan ICP over a KITTI-format sequence, consecutive pairs
// dealt round-robin over the GPUs of one node, ONE RCCL all-gather of the resulting SE(3) poses.
//
// Reference pieces either side of the registration path that this driver stands in for:
//   ros_node/kitti_reader.cc:91-149   `.bin` scans: float32 rows x y z reflectance, at most 1 000 000 floats per file,
//                                      files in sorted directory order
//   builder/map_builder.cc:354        pose_source = pose_target * align_result
//   builder/map_builder.cc:626-641    kitti_pose.txt: 12 floats per line (row-major top 3x4), setprecision(8)
// The reference itself has no multi-GPU path (its front end is one sequential thread); pairs are independent here because
// every pair's guess is fixed up front (identity or a constant forward step), as SURVEY.md §8(e) lays out.
//
// One process per GPU.  `smhip_shard --gpus G ...` re-executes itself G times (rank r on device r); the ranks can also be
// started by any launcher that sets RANK / WORLD_SIZE / LOCAL_RANK (torchrun's variables).  The ncclUniqueId travels from
// rank 0 to the others through a small file (--id-file, default under /tmp): no MPI, no sockets of our own.
// All arithmetic happens behind the C ABI of include/smhip.h; the gather is ncclAllGather on the doubles
// smhip_icp_export_results_device leaves in device memory -- the poses never visit the host before the collective.
//
// This file: the arguments, the id exchange, the alignment run (RunRank) and the launcher.  What rank 0 does after the run (--map,
// --submap-edges, --close-loops, --map-package) is shard_passes.h, each flag described at its pass; the poses, their product and the
// pose file's lines are shard_poses.h.
#include <dirent.h>
#include <fcntl.h>
#include <signal.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include "shard_passes.h"     // (and the standard headers)
#include "../../include/smhip/front_end.h"   // CtrvGuessFromLast

namespace {

using namespace shard;

constexpr int kPoseDoubles = 18;                 // 16 column-major transform + score + iterations

#define HIPOK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) Die(std::string(#e) + ": " + hipGetErrorString(e_)); } while (0)
#define NCCLOK(e) do { ncclResult_t r_ = (e); if (r_ != ncclSuccess) Die(std::string(#e) + ": " + ncclGetErrorString(r_)); } while (0)

std::vector<std::string> ListScans(const std::string& dir) {            // kitti_reader.cc:124-131: sorted listing
  std::vector<std::string> files;
  DIR* d = opendir(dir.c_str());
  if (!d) Die("cannot open " + dir);
  while (dirent* e = readdir(d)) {
    const std::string n = e->d_name;
    if (n.size() > 4 && n.compare(n.size() - 4, 4, ".bin") == 0) files.push_back(dir + "/" + n);
  }
  closedir(d);
  std::sort(files.begin(), files.end());
  return files;
}

// --gps-enu FILE into a->enu, before any device work: a line per scan of the listing, or the run ends here
void ReadGpsEnu(Args* a) {
  const size_t scans = ListScans(a->scans_dir).size();
  std::ifstream in(a->gps_enu);
  if (!in) Die("cannot read " + a->gps_enu);
  std::string text;
  while (std::getline(in, text)) {
    if (text.find_first_not_of(" \t\r") == std::string::npos) continue;
    std::array<double, 3> e;
    const char* p = text.c_str();
    for (int c = 0; c < 3; ++c) {
      char* end = nullptr;
      e[c] = std::strtod(p, &end);
      if (end == p) Die(a->gps_enu + ": line " + std::to_string(a->enu.size() + 1) + " does not hold three numbers");
      p = end;
    }
    a->enu.push_back(e);
  }
  if (a->enu.size() != scans)
    Die(a->gps_enu + " holds " + std::to_string(a->enu.size()) + " lines for " + std::to_string(scans) + " scans in " + a->scans_dir);
}

// --odom FILE into a->odom, before any device work: a line per scan of the listing with 12 numbers each, or the run ends here.  A line
// with a nan is "no reading"; the others are taken relative to the first of them.
void ReadOdom(Args* a) {
  const size_t scans = ListScans(a->scans_dir).size();
  std::ifstream in(a->odom_file);
  if (!in) Die("cannot read " + a->odom_file);
  std::string text;
  bool have_first = false;
  double fR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, ft[3] = {0, 0, 0};       // the first reading: rotation row-major, translation
  while (std::getline(in, text)) {
    if (text.find_first_not_of(" \t\r") == std::string::npos) continue;
    double m[12];
    const char* p = text.c_str();
    bool finite = true;
    for (int c = 0; c < 12; ++c) {
      char* end = nullptr;
      m[c] = std::strtod(p, &end);
      if (end == p) Die(a->odom_file + ": line " + std::to_string(a->odom.size() + 1) + " does not hold 12 numbers");
      finite = finite && std::isfinite(m[c]);
      p = end;
    }
    if (std::string(p).find_first_not_of(" \t\r") != std::string::npos) Die(a->odom_file + ": line " + std::to_string(a->odom.size() + 1) + " does not hold 12 numbers");
    std::array<double, 16> z{};                     // ([15] = 0: no reading)
    if (finite) {
      if (!have_first) { for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) fR[3 * r + c] = m[4 * r + c]; ft[r] = m[4 * r + 3]; } have_first = true; }
      for (int r = 0; r < 3; ++r) {                 // first^-1 * reading, column-major
        for (int c = 0; c < 3; ++c) z[4 * c + r] = fR[r] * m[c] + fR[3 + r] * m[4 + c] + fR[6 + r] * m[8 + c];
        z[12 + r] = fR[r] * (m[3] - ft[0]) + fR[3 + r] * (m[7] - ft[1]) + fR[6 + r] * (m[11] - ft[2]);
      }
      z[15] = 1.0;
    }
    a->odom.push_back(z);
  }
  if (a->odom.size() != scans)
    Die(a->odom_file + " holds " + std::to_string(a->odom.size()) + " lines for " + std::to_string(scans) + " scans in " + a->scans_dir);
}

Args Parse(int argc, char** argv) {
  Args a;
  for (int i = 1; i < argc; ++i) {
    const std::string k = argv[i];
    auto val = [&]() -> std::string { if (i + 1 >= argc) Die("missing value for " + k); return argv[++i]; };
    if (k == "--scans") a.scans_dir = val();
    else if (k == "--out") a.out_path = val();
    else if (k == "--gpus") a.gpus = std::atoi(val().c_str());
    else if (k == "--rank") a.rank = std::atoi(val().c_str());
    else if (k == "--world") a.world = std::atoi(val().c_str());
    else if (k == "--local-rank") a.local_rank = std::atoi(val().c_str());
    else if (k == "--id-file") a.id_file = val();
    else if (k == "--nonce") a.nonce = std::strtoull(val().c_str(), nullptr, 10);
    else if (k == "--batch") a.batch = std::atoi(val().c_str());
    else if (k == "--iterations") a.iterations = std::atoi(val().c_str());
    else if (k == "--early-exit") a.early_exit = std::atoi(val().c_str());
    else if (k == "--max-pairs") a.max_pairs = std::atoi(val().c_str());
    else if (k == "--readers") a.readers = std::atoi(val().c_str());
    else if (k == "--matchers") a.matchers = std::atoi(val().c_str());
    else if (k == "--warmup") a.warmup = std::atoi(val().c_str());
    else if (k == "--parts") a.parts = std::atoi(val().c_str());
    else if (k == "--guess-tx") a.guess_tx = std::atof(val().c_str());
    else if (k == "--guess") a.guess = val();
    else if (k == "--quiet") a.quiet = true;
    else if (k == "--map") a.map_path = val();
    else if (k == "--map-poses") a.map_poses = val();
    else if (k == "--map-every") a.map_every = std::atoi(val().c_str());
    else if (k == "--map-part-every") a.map_part_every = std::atoi(val().c_str());
    else if (k == "--map-resolution") a.map_resolution = static_cast<float>(std::atof(val().c_str()));
    else if (k == "--map-threshold") a.map_threshold = static_cast<float>(std::atof(val().c_str()));
    else if (k == "--map-hit") a.map_hit = static_cast<float>(std::atof(val().c_str()));
    else if (k == "--map-miss") a.map_miss = static_cast<float>(std::atof(val().c_str()));
    else if (k == "--map-points-per-cell") a.map_points_per_cell = std::atoi(val().c_str());
    else if (k == "--map-z-offset") a.map_z_offset = static_cast<float>(std::atof(val().c_str()));
    else if (k == "--map-average") a.map_average = true;
    else if (k == "--map-rgb") a.map_rgb = true;
    else if (k == "--map-max-table-log2") a.map_max_table_log2 = std::atoi(val().c_str());
    else if (k == "--map-compensate") { a.map_compensate = std::atoi(val().c_str()) != 0; a.map_compensate_given = true; }
    else if (k == "--map-package") a.map_package = val();
    else if (k == "--package-piece-width") a.package.piece_width = std::atof(val().c_str());
    else if (k == "--package-border-offset") a.package.border_offset = std::atof(val().c_str());
    else if (k == "--package-prefix") a.package.cloud_file_prefix = val();
    else if (k == "--package-descript") a.package.descript_filename = val();
    else if (k == "--submap-edges") a.submap_edges = val();
    else if (k == "--submap-frames") a.submap_frames = std::atoi(val().c_str());
    else if (k == "--submap-voxel") a.submap_voxel = static_cast<float>(std::atof(val().c_str()));
    else if (k == "--submap-min-score") a.submap_min_score = static_cast<float>(std::atof(val().c_str()));
    else if (k == "--close-loops") a.close_loops = val();
    else if (k == "--loop-ignore-threshold") a.loop.loop_ignore_threshold = std::atoi(val().c_str());
    else if (k == "--loop-detect-count") a.loop.trying_detect_loop_count = std::atoi(val().c_str());
    else if (k == "--loop-history") a.loop.nearest_history_pos_num = std::atoi(val().c_str());
    else if (k == "--loop-max-distance") a.loop.max_close_loop_distance = static_cast<float>(std::atof(val().c_str()));
    else if (k == "--loop-max-z") a.loop.max_close_loop_z_distance = static_cast<float>(std::atof(val().c_str()));
    else if (k == "--loop-use-descriptor") a.loop.use_descriptor = std::atoi(val().c_str()) != 0;
    else if (k == "--loop-m2dp-score") a.loop.m2dp_match_score = static_cast<float>(std::atof(val().c_str()));
    else if (k == "--loop-accept-score") a.loop.accept_scan_match_score = static_cast<float>(std::atof(val().c_str()));
    else if (k == "--loop-huber") {
      const std::string text = val();
      char* end = nullptr;
      a.loop_huber = std::strtod(text.c_str(), &end);
      if (text.empty() || *end != '\0') a.loop_huber = std::nan("");                  // (refused below)
      a.loop_huber_given = true;
    }
    else if (k == "--loop-report") a.loop_report = val();
    else if (k == "--loop-guess-search") { a.loop.guess_search = std::atoi(val().c_str()) != 0; a.loop_guess_given = true; }
    else if (k == "--loop-guess-resolution") { a.loop.guess_search_options.resolution = static_cast<float>(std::atof(val().c_str())); a.loop_guess_given = true; }
    else if (k == "--loop-guess-window") {
      int hxy = -1, hz = -1, steps = -1;
      double deg = std::nan("");
      if (std::sscanf(val().c_str(), "%d,%d,%d,%lf", &hxy, &hz, &steps, &deg) != 4) hxy = -1;             // (refused below)
      a.loop.guess_search_options.half_xy = hxy; a.loop.guess_search_options.half_z = hz; a.loop.guess_search_options.yaw_steps = steps;
      a.loop.guess_search_options.yaw_step = deg * M_PI / 180.0;
      a.loop_guess_given = true;
    }
    else if (k == "--pose-covariance") a.pose_covariance = val();
    else if (k == "--pose-covariance-chunk") a.pose_covariance_chunk = std::atoi(val().c_str());
    else if (k == "--pose-graph-dump") a.pose_graph_dump = val();
    else if (k == "--edge-information") { a.edge_information = std::atoi(val().c_str()) != 0; a.edge_information_given = true; }
    else if (k == "--edge-information-scale") {
      const std::string text = val();
      char* end = nullptr;
      a.edge_information_scale = std::strtod(text.c_str(), &end);
      if (text.empty() || *end != '\0') a.edge_information_scale = std::nan("");      // (refused below)
      a.edge_information_scale_given = true;
    }
    else if (k == "--edge-report") a.edge_report = val();
    else if (k == "--gps-enu") a.gps_enu = val();
    else if (k == "--gps-lever") { if (std::sscanf(val().c_str(), "%lf,%lf,%lf", &a.gps_lever[0], &a.gps_lever[1], &a.gps_lever[2]) != 3) Die("--gps-lever takes x,y,z"); }
    else if (k == "--gps-init-num") a.gps_init_num = std::atoi(val().c_str());
    else if (k == "--gps-sample-step") a.gps_sample_step = std::atoi(val().c_str());
    else if (k == "--gps-init-angle") a.gps_init_angle = std::atof(val().c_str());
    else if (k == "--gps-output-enu") a.gps_output_enu = true;
    else if (k == "--odom") a.odom_file = val();
    else if (k == "--odom-tf") {
      const std::string text = val();
      char tail = '\0';
      if (std::sscanf(text.c_str(), "%lf,%lf,%lf,%lf,%lf,%lf%c", &a.odom_tf[0], &a.odom_tf[1], &a.odom_tf[2], &a.odom_tf[3], &a.odom_tf[4], &a.odom_tf[5], &tail) != 6)
        a.odom_tf[0] = std::nan("");                                                     // (refused below)
      a.odom_tf_given = true;
    }
    else if (k == "--save-trajectory-map") a.save_trajectory_map = val();
    else if (k == "--join-base") a.join_base = val();
    else if (k == "--join-incremental") a.join_incremental = val();
    else if (k == "--join-out") a.join_out = val();
    else if (k == "--join-pcd") { a.join_pcd = val(); a.join_option_given = true; }
    else if (k == "--join-static-map") { a.join_static_map = val(); a.join_option_given = true; }
    else if (k == "--join-hold-base") { a.join_hold_base = std::atoi(val().c_str()) != 0; a.join_option_given = true; }
    else if (k == "--join-connection-huber") {
      const std::string text = val();
      char* end = nullptr;
      a.join_connection_huber = std::strtod(text.c_str(), &end);
      if (text.empty() || *end != '\0') a.join_connection_huber = std::nan("");        // (refused below)
      a.join_option_given = true;
    }
    else if (k == "--odom-calib") a.odom_calib = true;
    else if (k == "--odom-huber") {
      const std::string text = val();
      char* end = nullptr;
      a.odom_huber = std::strtod(text.c_str(), &end);
      if (text.empty() || *end != '\0') a.odom_huber = std::nan("");                  // (refused below)
      a.odom_huber_given = true;
    }
    else Die("unknown argument " + k + "\nusage: smhip_shard --scans DIR [--gpus G] [--out kitti_pose.txt] [--batch 256] "
             "[--iterations 20] [--early-exit 0|1] [--guess-tx metres] [--guess constant|ctrv (ctrv: pair k + 1 starts from pair k's motion; one GPU, one matcher)] [--max-pairs N] [--readers 8] [--matchers 1|2] [--warmup 1|0] [--parts 0..4]\n"
             "  static map: [--map map.pcd] [--map-poses kitti_pose.txt (map only)] [--map-every 1] [--map-part-every 0] [--map-resolution 0.1] "
             "[--map-threshold 0.6] [--map-hit 0.55] [--map-miss 0.48] [--map-points-per-cell 10] [--map-z-offset 0] [--map-average] [--map-rgb] "
             "[--map-max-table-log2 28] [--map-compensate 0|1 (with --map or --map-package: every frame de-skewed by its motion to the next pose of the file)]\n"
             "  map package: [--map-package DIR (from the poses as written, or --map-poses; submaps of --submap-frames frames at --submap-voxel, a "
             "trailing group that is not full is dropped; the pieces' maps take the --map-* settings)] [--package-piece-width 500] "
             "[--package-border-offset 100] [--package-prefix part_] [--package-descript map_package.xml]\n"
             "  submaps: [--submap-edges edges.txt] [--submap-frames 5] [--submap-voxel 0.1 (0: no voxel filter)] [--submap-min-score 0.7]\n"
             "  loop closing: [--close-loops corrected_pose.txt] [--loop-ignore-threshold 15] [--loop-detect-count 1] [--loop-history 4] "
             "[--loop-max-distance 25] [--loop-max-z 1] [--loop-use-descriptor 1] [--loop-m2dp-score 0.99] [--loop-accept-score 0.75] "
             "[--loop-huber 0 (the Huber threshold of the loop edges; 0: none)] [--loop-report FILE (a line per loop edge: target source norm weight)] "
             "[--loop-guess-search 1 (search a window around each candidate's pose-derived guess before its ICP; the report's lines gain "
             "search_score guess_score runner_up_score search_used)] [--loop-guess-resolution 0.5] [--loop-guess-window half_xy,half_z,yaw_steps,yaw_step_deg (20,2,10,2)] "
             "[--pose-covariance FILE (a line per submap: index held sigma_rot[3] sigma_pos_world[3] cov[21]) [--pose-covariance-chunk 256] [--pose-graph-dump FILE]]\n"
             "  edge information (with --close-loops): [--edge-information 1 (scan-match edges weighted by the matcher's own 6x6 information)] "
             "[--edge-information-scale 1] [--edge-report FILE (a line per edge: i j chain|loop kept residual_sigma strength[6] weakest[6])]\n"
             "  GPS (with --close-loops): [--gps-enu enu.txt (a line per scan: east north up in metres, nan = no fix)] [--gps-lever 0,0,0] "
             "[--gps-init-num 25] [--gps-sample-step 1] [--gps-init-angle 1.6] [--gps-output-enu (the poses in the ENU frame)]\n"
             "  odometry (with --close-loops): [--odom odom.txt (a line per scan: 12 numbers, the odometer's pose as a row-major 3x4, nan = no reading)] "
             "[--odom-tf 0,0,0,0,0,0 (odom -> lidar: tx,ty,tz,rx,ry,rz)] [--odom-calib (estimate it)] [--odom-huber 1]\n"
             "  a map to join later (with --close-loops): [--save-trajectory-map DIR (DIR/map.xml and a cloud file per submap)]\n"
             "  joining two maps (a run of its own, without --scans): --join-base A/map.xml --join-incremental B/map.xml --join-out C/map.xml "
             "[--join-hold-base 1] [--join-connection-huber 0] [--join-pcd whole.pcd] [--join-static-map static.pcd] [--loop-* as above; --loop-huber 1] [--loop-report FILE]");
  }
  if (a.guess != "constant" && a.guess != "ctrv") Die("--guess takes constant or ctrv (got " + a.guess + ")");
  if (a.Join()) {
    if (a.join_base.empty() || a.join_incremental.empty() || a.join_out.empty()) Die("a join takes --join-base, --join-incremental and --join-out together");
    if (!a.scans_dir.empty() || !a.close_loops.empty() || !a.map_path.empty() || !a.map_poses.empty() || !a.map_package.empty() || !a.submap_edges.empty())
      Die("a join is a run of its own: not with --scans, --map, --map-poses, --map-package, --submap-edges or --close-loops");
    if (!a.gps_enu.empty() || !a.odom_file.empty() || !a.save_trajectory_map.empty()) Die("a join takes no --gps-enu, --odom or --save-trajectory-map");
    if (!std::isfinite(a.join_connection_huber) || a.join_connection_huber < 0.0) Die("bad join setting (--join-connection-huber finite and >= 0)");
  } else if (a.join_option_given) {
    Die("--join-hold-base, --join-connection-huber, --join-pcd and --join-static-map need --join-base, --join-incremental and --join-out");
  }
  if (a.scans_dir.empty() && !a.Join()) Die("--scans DIR is required");
  if (!a.save_trajectory_map.empty() && a.close_loops.empty()) Die("--save-trajectory-map needs --close-loops");
  if (!a.map_poses.empty() && a.map_path.empty() && a.map_package.empty()) Die("--map-poses needs --map PATH");
  if (a.map_compensate_given && a.map_path.empty() && a.map_package.empty()) Die("--map-compensate needs --map or --map-package");
  if (!a.map_package.empty() && (!std::isfinite(a.package.piece_width) || !(a.package.piece_width > 0.0) || !std::isfinite(a.package.border_offset) ||
                                 a.package.descript_filename.empty()))
    Die("bad package setting (--package-piece-width finite and > 0, --package-border-offset finite, --package-descript not empty)");
  if (a.map_every < 1 || a.map_part_every < 0 || a.map_points_per_cell < 1 || a.map_max_table_log2 < 10 || a.map_max_table_log2 > 28 ||
      !(a.map_resolution > 0.f))
    Die("bad map setting (--map-every >= 1, --map-part-every >= 0, --map-points-per-cell >= 1, --map-max-table-log2 10..28, --map-resolution > 0)");
  if (a.submap_frames < 1 || !(a.submap_voxel >= 0.f) || !std::isfinite(a.submap_voxel))
    Die("bad submap setting (--submap-frames >= 1, --submap-voxel >= 0)");
  if (!a.submap_edges.empty() && !a.map_poses.empty()) Die("--submap-edges needs the alignment run (not --map-poses)");
  if (!a.close_loops.empty() && !a.map_poses.empty()) Die("--close-loops needs the alignment run (not --map-poses)");
  if (!a.gps_enu.empty() && a.close_loops.empty()) Die("--gps-enu needs --close-loops");
  if (a.loop_huber_given && a.close_loops.empty() && !a.Join()) Die("--loop-huber needs --close-loops");
  if (!a.loop_report.empty() && a.close_loops.empty() && !a.Join()) Die("--loop-report needs --close-loops");
  if (a.loop_guess_given && a.close_loops.empty() && !a.Join()) Die("--loop-guess-search, --loop-guess-resolution and --loop-guess-window need --close-loops");
  if (a.loop_guess_given) {
    const smhip_guess_search_options& g = a.loop.guess_search_options;
    if (!std::isfinite(g.resolution) || !(g.resolution > 0.f) || g.half_xy < 0 || g.half_z < 0 || g.yaw_steps < 0 || !std::isfinite(g.yaw_step))
      Die("bad guess search (--loop-guess-resolution finite and > 0, --loop-guess-window half_xy,half_z,yaw_steps,yaw_step_deg, none negative)");
  }
  if (!a.pose_covariance.empty() && a.close_loops.empty()) Die("--pose-covariance needs --close-loops");
  if ((!a.pose_graph_dump.empty() || a.pose_covariance_chunk != 256) && a.pose_covariance.empty()) Die("--pose-graph-dump and --pose-covariance-chunk need --pose-covariance");
  if (a.pose_covariance_chunk < 1) Die("--pose-covariance-chunk takes a count of at least 1");
  for (const std::string* path : {&a.pose_covariance, &a.pose_graph_dump})      // before any work, and without touching the file
    if (!path->empty() && !CanWrite(*path)) Die("cannot write " + *path);
  if ((a.edge_information_given || a.edge_information_scale_given || !a.edge_report.empty()) && a.close_loops.empty())
    Die("--edge-information, --edge-information-scale and --edge-report need --close-loops");
  if ((a.edge_information_scale_given || !a.edge_report.empty()) && !a.edge_information) Die("--edge-information-scale and --edge-report need --edge-information 1");
  if (!std::isfinite(a.edge_information_scale) || !(a.edge_information_scale > 0.0)) Die("bad edge setting (--edge-information-scale finite and > 0)");
  if (a.gps_output_enu && a.gps_enu.empty()) Die("--gps-output-enu needs --gps-enu");
  if (!a.odom_file.empty() && a.close_loops.empty()) Die("--odom needs --close-loops");
  if ((a.odom_tf_given || a.odom_calib || a.odom_huber_given) && a.odom_file.empty()) Die("--odom-tf, --odom-calib and --odom-huber need --odom");
  for (int c = 0; c < 6; ++c) if (!std::isfinite(a.odom_tf[c])) Die("bad odometry setting (--odom-tf takes tx,ty,tz,rx,ry,rz, all finite)");
  if (!std::isfinite(a.odom_huber) || a.odom_huber < 0.0) Die("bad odometry setting (--odom-huber finite and >= 0)");
  if (!std::isfinite(a.gps_lever[0]) || !std::isfinite(a.gps_lever[1]) || !std::isfinite(a.gps_lever[2]) || !std::isfinite(a.gps_init_angle) || a.gps_init_num < 0)
    Die("bad GPS setting (--gps-lever finite, --gps-init-angle finite, --gps-init-num >= 0)");
  if (a.loop.nearest_history_pos_num < 1 || a.loop.loop_ignore_threshold < 0 || a.loop.trying_detect_loop_count < 1)
    Die("bad loop setting (--loop-history >= 1, --loop-ignore-threshold >= 0, --loop-detect-count >= 1)");
  if (!std::isfinite(a.loop_huber) || a.loop_huber < 0.0) Die("bad loop setting (--loop-huber finite and >= 0)");
  if (a.rank < 0 && std::getenv("RANK")) a.rank = std::atoi(std::getenv("RANK"));
  if (a.world < 0 && std::getenv("WORLD_SIZE")) a.world = std::atoi(std::getenv("WORLD_SIZE"));
  if (a.local_rank < 0 && std::getenv("LOCAL_RANK")) a.local_rank = std::atoi(std::getenv("LOCAL_RANK"));
  // a pair's guess comes from its predecessor's result: round-robin pairs have none on their rank, and a second matcher would run beside it
  // (after the launcher's variables are read: WORLD_SIZE counts as --world)
  if (a.guess == "ctrv" && (a.gpus > 1 || a.world > 1)) Die("--guess ctrv runs on one GPU (not with --gpus " + std::to_string(std::max(a.gpus, a.world)) + ")");
  if (a.guess == "ctrv" && a.matchers >= 2) Die("--guess ctrv runs one matcher (not with --matchers " + std::to_string(a.matchers) + ")");
  return a;
}

// rank 0 creates the communicator id and publishes it; the others wait for the file.  The file carries a per-run nonce
// (the launcher's, or MASTER_PORT / SMHIP_SHARD_NONCE under an external launcher) in front of the id: a file left behind by
// a crashed run -- or by another run using the same path -- does not match and is waited out instead of being taken for
// this run's id (ncclCommInitRank would hang on a stale one).  Rank 0 replaces any existing file (unlink + O_EXCL on the
// temporary, then rename) and removes it at exit, also on the error paths.
struct IdRecord { unsigned long long nonce; ncclUniqueId id; };
std::string g_id_file_to_remove;
void RemoveIdFile() { if (!g_id_file_to_remove.empty()) std::remove(g_id_file_to_remove.c_str()); }

ncclUniqueId ExchangeId(const Args& a, int rank) {
  IdRecord rec{};
  rec.nonce = a.nonce;
  if (rank == 0) {
    NCCLOK(ncclGetUniqueId(&rec.id));
    const std::string tmp = a.id_file + ".tmp." + std::to_string(static_cast<long>(getpid()));
    std::remove(a.id_file.c_str());
    std::remove(tmp.c_str());
    const int fd = open(tmp.c_str(), O_CREAT | O_EXCL | O_WRONLY, 0600);
    if (fd < 0) Die("cannot create " + tmp);
    const bool ok = write(fd, &rec, sizeof(rec)) == static_cast<ssize_t>(sizeof(rec));
    close(fd);
    if (!ok) { std::remove(tmp.c_str()); Die("cannot write " + tmp); }
    g_id_file_to_remove = a.id_file;
    std::atexit(RemoveIdFile);
    if (std::rename(tmp.c_str(), a.id_file.c_str()) != 0) { std::remove(tmp.c_str()); Die("cannot publish " + a.id_file); }
    return rec.id;
  }
  for (int tries = 0; tries < 6000; ++tries) {                           // <= 60 s
    IdRecord got{};
    std::ifstream f(a.id_file, std::ios::binary);
    if (f && f.read(reinterpret_cast<char*>(&got), sizeof(got)) && f.gcount() == static_cast<std::streamsize>(sizeof(got)) &&
        got.nonce == a.nonce)
      return got.id;
    usleep(10000);
  }
  Die("timed out waiting for " + a.id_file + " (no file with this run's nonce appeared)");
}

// --map-poses FILE: the map alone, one process, no alignment and no RCCL.  The pose file is checked before any GPU work: it needs
// a pose for every frame the map inserts.
int RunMapOnly(const Args& a) {
  const auto files = ListScans(a.scans_dir);
  int n_frames = static_cast<int>(files.size());
  if (a.max_pairs > 0) n_frames = std::min(n_frames, a.max_pairs + 1);
  std::vector<Pose> poses;
  if (!ReadPoses(a.map_poses, &poses)) Die("cannot open " + a.map_poses);
  const std::vector<int> frames = MapFrames(a, n_frames);
  if (frames.empty()) Die("no scans in " + a.scans_dir);
  if (!a.map_path.empty() && static_cast<int>(poses.size()) <= frames.back())
    Die(a.map_poses + " holds " + std::to_string(poses.size()) + " poses; the map needs one for every frame up to " + std::to_string(frames.back()) +
        " (" + std::to_string(frames.back() + 1) + " lines)");
  const int package_frames = n_frames / a.submap_frames * a.submap_frames;          // the frames of the full submaps
  if (!a.map_package.empty() && static_cast<int>(poses.size()) < package_frames)
    Die(a.map_poses + " holds " + std::to_string(poses.size()) + " poses; the map package needs one for each of the first " + std::to_string(package_frames) + " frames");
  std::string fields;
  const int rc = RunPasses(a, files, n_frames, poses, 0, &fields);     // (Parse left --map and --map-package only)
  if (rc == 0 && !a.quiet)
    std::printf("%s}\n", (Fmt("{\"driver\": \"smhip_shard (map only)\", \"poses_file\": \"%s\", \"poses_in_file\": %d", a.map_poses.c_str(),
                              static_cast<int>(poses.size())) + fields).c_str());
  return rc;
}

int RunRank(const Args& a, int rank, int world, int device) {
  const auto files = ListScans(a.scans_dir);
  if (files.size() < 2) Die("need at least two scans in " + a.scans_dir);
  int n_pairs = static_cast<int>(files.size()) - 1;
  if (a.max_pairs > 0) n_pairs = std::min(n_pairs, a.max_pairs);
  const int per = (n_pairs + world - 1) / world;                         // padded pairs per rank
  // a scan without a point (an empty or cut-off file; the upload refuses n <= 0 without knowing the file) ends the run by name,
  // before any device work
  for (int k = 0; k <= n_pairs; ++k) {
    struct stat sb;
    if (stat(files[k].c_str(), &sb) == 0 && sb.st_size < 16)
      Die(files[k] + " holds no point (" + std::to_string(static_cast<long long>(sb.st_size)) + " bytes; a row is 16)");
  }

  HIPOK(hipSetDevice(device));
  ncclComm_t comm;
  const ncclUniqueId id = ExchangeId(a, rank);
  NCCLOK(ncclCommInitRank(&comm, world, id, rank));

  const int B = std::max(1, std::min(std::min(a.batch, 256), per));     // one batched upload holds up to 2 B <= 512 scans
  // --matchers 2: two matchers, each with its own stream, take the batches in turn -- while one runs the alignments of batch k
  // (enqueued, not waited for), the host reads, uploads and prepares the targets of batch k + 1 on the other.
  const int NH = (a.matchers >= 2 && per > B) ? 2 : 1;
  // --guess ctrv (one rank, one matcher): reading, the batched upload and the forest pass as they are; the pairs of a batch are then
  // aligned one after the other, each a single-pair Align (the cooperative launch), pair k + 1 from front_end::CtrvGuessFromLast of
  // pair k's result on the host -- across batches too.  (Parse refuses more than one rank.)
  const bool ctrv = a.guess == "ctrv";
  smhip::registrator::Matrix4d ctrv_guess = smhip::registrator::Matrix4d::Identity();
  ctrv_guess(0, 3) = a.guess_tx;
  hipStream_t streams[2] = {nullptr, nullptr};
  smhip_handle hs[2] = {nullptr, nullptr};
  for (int k = 0; k < NH; ++k) HIPOK(hipStreamCreateWithFlags(&streams[k], hipStreamNonBlocking));
  hipStream_t stream = streams[0];
  // capacity: the largest scan of the directory (a KITTI scan holds at most 250 000 points: 1 000 000 floats per file are
  // read, kitti_reader.cc:93).  Slots [0, B) hold the pairs of a batch, slots [B, 2 B) park target scans that no pair of the
  // batch holds as its source already.
  size_t max_bytes = 16;
  for (const auto& f : files) { struct stat sb; if (stat(f.c_str(), &sb) == 0) max_bytes = std::max(max_bytes, static_cast<size_t>(sb.st_size)); }
  const size_t slot_floats = SlotFloats(max_bytes);
  const int cap = static_cast<int>(slot_floats / 4);
  for (int k = 0; k < NH; ++k) {
    const smhip_status s = smhip_create(device, streams[k], 2 * B, cap, cap, &hs[k]);
    if (s != SMHIP_OK) Die(std::string("smhip_create: ") + smhip_status_string(s) + " (is this a gfx950 GPU? there is no CPU fallback)");
    smhip_icp_options o;
    smhip_icp_default_options(&o);
    o.max_iteration = a.iterations;
    o.early_exit = a.early_exit;
    if (a.parts > 0) o.overlap_streams = a.parts;         // parts of a batch on streams of their own (0: the library's default, two)
    if (smhip_icp_set_options(hs[k], &o) != SMHIP_OK) Die(smhip_last_error(hs[k]));
  }

  double* local_dev = nullptr;
  double* all_dev = nullptr;
  HIPOK(hipMalloc(reinterpret_cast<void**>(&local_dev), sizeof(double) * kPoseDoubles * per));
  HIPOK(hipMalloc(reinterpret_cast<void**>(&all_dev), sizeof(double) * kPoseDoubles * per * world));
  HIPOK(hipMemsetAsync(local_dev, 0, sizeof(double) * kPoseDoubles * per, stream));

  // guess: column-major 4x4; identity or a constant forward step (SURVEY.md §8(d) cfg 4; the reference front end always
  // hands its matcher an extrapolated pose, map_builder.cc:302-308)
  std::vector<double> guesses(16 * static_cast<size_t>(B), 0.0);
  for (int k = 0; k < B; ++k) { double* g = &guesses[16 * static_cast<size_t>(k)]; g[0] = g[5] = g[10] = g[15] = 1.0; g[12] = a.guess_tx; }

  // the files this rank reads, in reading order (the same walk as the loop below)
  const std::vector<int> order = smhip::kitti::ShardReadOrder(n_pairs, world, rank, B);
  // The readers fill page-locked buffers and the batch's uploads are DMA'd straight out of them (no staging copy): a
  // buffer is held from Next() until the uploads of its batch have left the host (ReleaseHeld), so the ring holds two
  // batches' worth of scans -- one being uploaded, one being read ahead.
  const int scans_per_batch = world == 1 ? B + 1 : 2 * B;
  const int ring = 2 * scans_per_batch + std::max(1, a.readers);
  std::vector<float*> ring_buffers(ring, nullptr);
  bool pinned = true;
  for (int k = 0; k < ring && pinned; ++k)
    if (hipHostMalloc(reinterpret_cast<void**>(&ring_buffers[k]), slot_floats * sizeof(float), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); pinned = false; }
  std::vector<std::vector<float>> pageable;                  // the host refused that much page-locked memory: ordinary buffers, staged uploads
  if (!pinned) {
    for (float*& b : ring_buffers) { if (b) (void)hipHostFree(b); b = nullptr; }
    pageable.assign(ring, std::vector<float>(slot_floats));
    for (int k = 0; k < ring; ++k) ring_buffers[k] = pageable[k].data();
  }
  for (int k = 0; k < NH; ++k) {
    if (smhip_reserve_batch_workspaces(hs[k]) != SMHIP_OK) Die(smhip_last_error(hs[k]));     // not inside the first batch
    HIPOK(hipStreamSynchronize(streams[k]));
  }
  // Part of bringing the process up, like the handle and its workspaces above: one batch of 32 small made-up scans (three walls of a
  // room, 8 192 points each) through the same four calls as every batch below.  The first use of a kernel loads its code object, the
  // first batched upload creates the copy stream, the first radix sort sizes rocPRIM's workspace -- 25 ms of a first batch that a
  // mapping process pays once, not per sequence.  Nothing of it survives: every slot is set again by the first real batch.
  double warmup_s = 0.0;
  if (a.warmup) {
    const auto w0 = std::chrono::steady_clock::now();
    const int WN = 8192, WS = std::min(32, B);
    // (page-locked like the readers' buffers, so that the upload takes the same road)
    float* wmem = nullptr;
    std::vector<float> wpageable;
    const size_t wfloats = 4 * static_cast<size_t>(WN);
    if (!pinned || hipHostMalloc(reinterpret_cast<void**>(&wmem), wfloats * (WS + 1) * sizeof(float), hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError(); wmem = nullptr; wpageable.resize(wfloats * (WS + 1));
    }
    float* wbase = wmem ? wmem : wpageable.data();
    std::vector<float*> wscan(WS + 1);
    for (int k = 0; k <= WS; ++k) wscan[k] = wbase + wfloats * k;
    uint32_t lcg = 12345u;
    auto u01 = [&]() { lcg = lcg * 1664525u + 1013904223u; return static_cast<float>(lcg >> 8) * (1.0f / 16777216.0f); };
    for (int k = 0; k <= WS; ++k)
      for (int i = 0; i < WN; ++i) {
        float x = 20.f * u01() - 10.f, y = 20.f * u01() - 10.f, z = 4.f * u01();
        switch (i % 3) { case 0: z = 0.002f * u01(); break; case 1: x = 10.f + 0.002f * u01(); break; default: y = 10.f + 0.002f * u01(); break; }
        float* r = &wscan[k][4 * static_cast<size_t>(i)];
        r[0] = x - 0.02f * k; r[1] = y; r[2] = z; r[3] = 0.f;
      }
    for (int hk = 0; hk < NH; ++hk) {
      std::vector<int> wslots, wn, wfrom, wto, wnt(WS);
      std::vector<const float*> wrows;
      wrows.push_back(wscan[0]); wslots.push_back(B); wn.push_back(WN); wfrom.push_back(B); wto.push_back(0);
      for (int k = 0; k < WS; ++k) {
        wrows.push_back(wscan[k + 1]); wslots.push_back(k); wn.push_back(WN);
        if (k > 0) { wfrom.push_back(k - 1); wto.push_back(k); }
      }
      if (smhip_set_sources_f32_batch(hs[hk], static_cast<int>(wslots.size()), wslots.data(), wrows.data(), wn.data()) != SMHIP_OK ||
          smhip_prepare_targets_from_sources(hs[hk], WS, wfrom.data(), wto.data(), wnt.data()) != SMHIP_OK ||
          smhip_icp_enqueue_batch(hs[hk], WS, guesses.data()) != SMHIP_OK ||
          smhip_icp_export_results_device(hs[hk], WS, local_dev) != SMHIP_OK ||
          // (what the made-up batch taught the handle about where to switch search forms is forgotten: the first real batch chooses
          // as it does without the warm-up)
          smhip_icp_forget_search_history(hs[hk]) != SMHIP_OK)
        Die(std::string("warm-up batch: ") + smhip_last_error(hs[hk]));
      HIPOK(hipStreamSynchronize(streams[hk]));
    }
    HIPOK(hipMemsetAsync(local_dev, 0, sizeof(double) * kPoseDoubles * per, stream));
    HIPOK(hipStreamSynchronize(stream));
    if (wmem) (void)hipHostFree(wmem);
    warmup_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - w0).count();
  }
  // the clock starts BEFORE the first file is opened: the readers start here (their head start used to be whatever the set-up above took)
  const auto t0 = std::chrono::steady_clock::now();
  ScanPrefetcher scans(files, order, a.readers, ring_buffers, slot_floats, /*hold_until_release=*/true);
  auto next_scan = [&](int expect, int* n) -> const float* {
    int fi = -1;
    const float* rows = scans.Next(n, &fi);
    if (!rows || fi != expect) Die("prefetcher out of step with the batch loop");
    if (*n < 0) Die("cannot read " + files[fi]);
    if (*n == 0) Die(files[fi] + " holds no point");
    // A scan without one finite point has no target and no correspondence: CalculateNormals would drop every leaf ("produced no
    // target points") after building a tree over one run of equal keys.  Ended here by name instead; an ordinary scan leaves the
    // loop at its first row.
    bool finite = false;
    for (int i = 0; i < *n && !finite; ++i)
      finite = std::isfinite(rows[4 * static_cast<size_t>(i)]) && std::isfinite(rows[4 * static_cast<size_t>(i) + 1]) && std::isfinite(rows[4 * static_cast<size_t>(i) + 2]);
    if (!finite) Die(files[fi] + " holds no finite point");
    return rows;
  };
  double upload_s = 0.0, wait_s = 0.0, set_s = 0.0, prep_s = 0.0;   // rank 0's host-side split: blocked on the readers / uploads / target preparation
  auto since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); };
  int my_pairs = 0;
  // the batch period once the pipeline is full: from the first batch's alignments being enqueued to the last batch's, over the pairs of
  // the batches after the first (a run of four batches spends a quarter of its time filling and draining)
  double first_enq_s = 0.0, last_enq_s = 0.0;
  int first_enq_pairs = 0, enq_pairs = 0;
  // SMHIP_SHARD_TIMELINE=1: where the host is (ms since the clock started) as it walks a batch -- to lay next to a kernel trace
  const bool timeline = rank == 0 && std::getenv("SMHIP_SHARD_TIMELINE") != nullptr;
  auto mark = [&](const char* what, int base) { if (timeline) std::fprintf(stderr, "[timeline] %8.3f ms  batch at %d: %s\n", since(t0) * 1e3, base, what); };
  std::vector<int> up_slots, up_n;
  std::vector<const float*> up_rows;
  for (int base = 0, turn = 0; base < per; base += B, ++turn) {
    smhip_handle h = hs[turn % NH];
    int nb = 0;
    const auto u0 = std::chrono::steady_clock::now();
    std::vector<int> from, to, nts;
    up_slots.clear(); up_n.clear(); up_rows.clear();
    int prev_pair = -2;
    auto w0 = std::chrono::steady_clock::now();
    for (int k = 0; k < B && base + k < per; ++k) {
      const int pair = (base + k) * world + rank;                        // round-robin: pair i -> rank i mod G
      if (pair >= n_pairs) break;
      // scan i = target.  When the previous slot's pair is i - 1 its source IS scan i, already part of this upload (one GPU:
      // every pair but the first of a batch); otherwise the scan is parked in slot B + k.  Either way the scans of the whole
      // batch go up in ONE call and its targets are prepared in ONE device pass (CalculateNormals as a forest of kd-trees).
      if (pair == prev_pair + 1) from.push_back(k - 1);
      else {
        int n = 0;
        up_rows.push_back(next_scan(pair, &n)); up_slots.push_back(B + k); up_n.push_back(n);
        from.push_back(B + k);
      }
      to.push_back(k);
      int n = 0;
      up_rows.push_back(next_scan(pair + 1, &n)); up_slots.push_back(k); up_n.push_back(n);   // scan i + 1 = source
      prev_pair = pair;
      ++nb;
    }
    wait_s += since(w0);
    if (nb == 0) break;
    mark("scans at hand", base);
    w0 = std::chrono::steady_clock::now();
    if (smhip_set_sources_f32_batch(h, static_cast<int>(up_slots.size()), up_slots.data(), up_rows.data(), up_n.data()) != SMHIP_OK)
      Die(std::string("upload of batch at pair ") + std::to_string(base * world + rank) + ": " + smhip_last_error(h));
    set_s += since(w0);
    mark("upload + ordering enqueued", base);
    nts.resize(nb);
    {
      w0 = std::chrono::steady_clock::now();
      if (smhip_prepare_targets_from_sources(h, nb, from.data(), to.data(), nts.data()) != SMHIP_OK) Die(std::string("prepare targets: ") + smhip_last_error(h));
      prep_s += since(w0);
      mark("targets prepared (blocking)", base);
    }
    scans.ReleaseHeld();            // prepare_targets blocked on the stream: the uploads have left the host buffers
    upload_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - u0).count();
    if (ctrv) {
      for (int k = 0; k < nb; ++k) {
        smhip::registrator::Matrix4d result = ctrv_guess;                // (a pair without a correspondence keeps its guess)
        double score = 0.0;
        const smhip_status st = smhip_icp_align_range(h, k, 1, ctrv_guess.data(), result.data(), &score, nullptr);
        // a pair that failed as a pair is counted below from its exported row (0 iterations); anything else ends the run
        if (st != SMHIP_OK && st != SMHIP_ERR_NO_MATCH && st != SMHIP_ERR_INVALID_ARGUMENT) Die(std::string("align pair ") + std::to_string(base + k) + ": " + smhip_last_error(h));
        ctrv_guess = smhip::front_end::CtrvGuessFromLast(result);
      }
    } else if (smhip_icp_enqueue_batch(h, nb, guesses.data()) != SMHIP_OK) Die(std::string("enqueue: ") + smhip_last_error(h));
    if (smhip_icp_export_results_device(h, nb, local_dev + static_cast<size_t>(kPoseDoubles) * base) != SMHIP_OK) Die(smhip_last_error(h));
    mark("alignments enqueued", base);
    if (turn == 0) { first_enq_s = since(t0); first_enq_pairs = nb; }
    last_enq_s = since(t0); enq_pairs += nb;
    my_pairs += nb;
  }
  for (int k = 1; k < NH; ++k) HIPOK(hipStreamSynchronize(streams[k]));     // (the gather goes to the first matcher's stream)
  // the ONE collective of the path: every rank's padded block of poses, device to device over xGMI
  NCCLOK(ncclAllGather(local_dev, all_dev, static_cast<size_t>(kPoseDoubles) * per, ncclDouble, comm, stream));
  HIPOK(hipStreamSynchronize(stream));
  const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  int rc = 0;
  std::string line;                                                      // rank 0's summary, printed after the map phase with --map
  if (rank == 0) {
    std::vector<double> all(static_cast<size_t>(kPoseDoubles) * per * world);
    HIPOK(hipMemcpy(all.data(), all_dev, sizeof(double) * all.size(), hipMemcpyDeviceToHost));
    // rank r, local slot s -> pair s * world + r;  chain pose_{i+1} = pose_i * T_i
    std::ofstream out(a.out_path);
    if (!out) Die("cannot write " + a.out_path);
    out.precision(8);
    Pose pose{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    WritePoseLine(out, pose.data());
    double score_sum = 0.0, iter_sum = 0.0;
    int bad = 0;
    for (int pair = 0; pair < n_pairs; ++pair) {
      const double* row = &all[static_cast<size_t>(kPoseDoubles) * (static_cast<size_t>(pair % world) * per + pair / world)];
      Pose T;
      std::copy(row, row + 16, T.begin());
      if (!(row[17] >= 1.0)) ++bad;                                      // a pair that never ran left zeros; one that failed exports 0 iterations (smhip.h)
      pose = MulPose(pose, T);
      WritePoseLine(out, pose.data());
      score_sum += row[16]; iter_sum += row[17];
    }
    out.close();
    if (!a.quiet || bad) {
      line = Fmt("{\"driver\": \"smhip_shard (C++, RCCL all-gather)\", \"n_gpus\": %d, \"pairs\": %d, \"pairs_rank0\": %d, \"seconds\": %.4f, "
                  "\"pairs_per_s\": %.2f, \"read_upload_prepare_s_rank0\": %.4f, \"wait_for_readers_s_rank0\": %.4f, \"upload_s_rank0\": %.4f, "
                  "\"prepare_targets_s_rank0\": %.4f, \"mean_score\": %.6f, \"mean_iterations\": %.2f, "
                  "\"unfinished_pairs\": %d, \"batch\": %d, \"readers\": %d, \"pinned_read_buffers\": %s, \"warmup_batch_before_the_clock_s\": %.4f, \"steady_state_pairs_per_s_rank0\": %.2f, \"poses_file\": \"%s\"",
                  world, n_pairs, my_pairs, elapsed, n_pairs / elapsed, upload_s, wait_s, set_s, prep_s, score_sum / n_pairs, iter_sum / n_pairs, bad, B, a.readers, pinned ? "true" : "false", warmup_s,
                  last_enq_s > first_enq_s ? (enq_pairs - first_enq_pairs) / (last_enq_s - first_enq_s) : 0.0, a.out_path.c_str());
      if (ctrv) line += ", \"guess\": \"ctrv\"";
      if (!AnyPass(a)) { std::printf("%s}\n", line.c_str()); line.clear(); }
    }
    if (bad) rc = 3;
  }
  (void)hipFree(local_dev); (void)hipFree(all_dev);
  for (int k = 0; k < NH; ++k) smhip_destroy(hs[k]);
  if (pinned) for (float* b : ring_buffers) (void)hipHostFree(b);
  NCCLOK(ncclCommDestroy(comm));
  for (int k = 0; k < NH; ++k) (void)hipStreamDestroy(streams[k]);
  if (rank == 0 && AnyPass(a)) {
    // from the poses as written: the pose file read back (--map-poses on that file builds the same map)
    std::string fields;
    std::vector<Pose> poses;
    if (rc == 0 && (!ReadPoses(a.out_path, &poses) || static_cast<int>(poses.size()) != n_pairs + 1)) Die("cannot read back " + a.out_path);
    if (rc == 0) rc = RunPasses(a, files, n_pairs + 1, poses, device, &fields);
    if (!line.empty()) std::printf("%s%s}\n", line.c_str(), rc == 0 ? fields.c_str() : "");
  }
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  // the library splits a batch over up to four streams and RCCL brings its own: more hardware queues than the runtime's default 4, or
  // two of them share a queue and run one after the other (as bench.py does; must be set before the runtime starts)
  setenv("GPU_MAX_HW_QUEUES", "8", 0);
  Args a = Parse(argc, argv);
  if (!a.gps_enu.empty()) ReadGpsEnu(&a);
  if (!a.odom_file.empty()) ReadOdom(&a);
  if (a.Join()) return JoinMaps(a, 0);                                   // joining two maps: one process, no scans, no RCCL
  if (a.id_file.empty()) a.id_file = "/tmp/smhip_shard_id_" + std::to_string(a.rank >= 0 ? static_cast<long>(getppid()) : static_cast<long>(getpid()));
  if (!a.map_poses.empty()) return RunMapOnly(a);                       // the map alone: one process, no RCCL
  if (a.rank >= 0) {                                                     // one rank of a launched group
    const int world = a.world > 0 ? a.world : 1;
    if (a.nonce == 0) {                                                  // external launcher: every rank sees the same MASTER_PORT
      const char* e = std::getenv("SMHIP_SHARD_NONCE");
      if (!e) e = std::getenv("MASTER_PORT");
      if (e) a.nonce = std::strtoull(e, nullptr, 10);
    }
    return RunRank(a, a.rank, world, a.local_rank >= 0 ? a.local_rank : a.rank);
  }
  a.nonce = (static_cast<unsigned long long>(getpid()) << 32) ^ static_cast<unsigned long long>(std::chrono::steady_clock::now().time_since_epoch().count());
  if (a.gpus <= 1) return RunRank(a, 0, 1, 0);
  // launcher: one child process per GPU (fresh processes -- no HIP state is inherited across the fork)
  std::remove(a.id_file.c_str());
  std::vector<pid_t> kids;
  for (int r = 0; r < a.gpus; ++r) {
    const pid_t pid = fork();
    if (pid < 0) { for (pid_t k : kids) kill(k, SIGTERM); Die("fork failed"); }
    if (pid == 0) {
      std::vector<std::string> args(argv, argv + argc);
      args.push_back("--rank"); args.push_back(std::to_string(r));
      args.push_back("--world"); args.push_back(std::to_string(a.gpus));
      args.push_back("--local-rank"); args.push_back(std::to_string(r));
      args.push_back("--id-file"); args.push_back(a.id_file);
      args.push_back("--nonce"); args.push_back(std::to_string(a.nonce));
      std::vector<char*> cargs;
      for (auto& s : args) cargs.push_back(const_cast<char*>(s.c_str()));
      cargs.push_back(nullptr);
      execv("/proc/self/exe", cargs.data());
      std::perror("execv");
      _exit(127);
    }
    kids.push_back(pid);
  }
  // a rank that dies before the all-gather (unreadable scan, device error) would leave the others blocked in it for good:
  // the first failure ends the whole group
  int rc = 0;
  size_t left = kids.size();
  while (left > 0) {
    int st = 0;
    const pid_t k = waitpid(-1, &st, 0);
    if (k < 0) break;
    --left;
    const int code = WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0);
    if (code != 0 && rc == 0) {
      rc = code;
      for (pid_t other : kids) if (other != k) kill(other, SIGTERM);
    }
  }
  std::remove(a.id_file.c_str());
  return rc;
}
