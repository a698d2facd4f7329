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
// --map PATH: the static map of MapBuilder::SaveMaps (builder/map_builder.cc:825-910).  Once kitti_pose.txt is written and the
// matchers are gone, rank 0 reads the scans again in order and inserts frame k under pose k into one device
// MultiResolutionVoxelMap (ApplyTransformToOutput on the device, origin = the pose's translation), then writes PATH as a PCD
// file with rows in voxel-key order.  The poses are the ones AS WRITTEN to the pose file (8 significant digits, parsed back),
// so the map is a function of that file: --map-poses FILE builds the same map, byte for byte, with no alignment, no RCCL and
// one process -- also from poses that came from elsewhere.
//
// --close-loops PATH: the pose graph over those submaps (MapBuilder::ConnectAllSubmap, builder/map_builder.cc:448-613): every submap
// with its device descriptor goes through back_end::IsamOptimizer (smhip/pose_graph.h: the loop detector, consecutive matches as
// odometry factors, loop edges, one device solve per update), and the frames' corrected poses are written to PATH in the pose
// writer's format, one line per frame -- so --map --map-poses PATH builds the corrected map.  The detector's settings are the
// --loop-* flags (back_end/loop_detector_options.h:29-40).  Without the flag nothing of this runs and every output is what it was.
// With --gps-enu FILE (one line per scan in file order: east north up in metres, nan = no fix; the geodetic conversion is not
// restated) a submap carries the fix of its first frame and IsamOptimizer adds the GPS / ENU factors of isam_optimizer.cc:238-349
// (--gps-lever x,y,z: the antenna in the tracking frame; --gps-init-num, --gps-sample-step, --gps-init-angle: isam_optimizer.h:61-66);
// --gps-output-enu premultiplies every submap pose by GetGpsCoordTransform() before UpdateInnerFramePose (map_builder.cc:748-762),
// so PATH is in the ENU frame.  --gps-enu without --close-loops, or a FILE whose line count is not the scan count, ends the run
// with exit 2 before any device work.
//
// --map-package DIR: the map package of MapBuilder::SaveMapPackage (builder/map_builder.cc:816-823, builder/map_package.cc): the
// static map cut into overlapping square pieces, DIR/<prefix><x>_<y>.pcd centred on the piece and DIR/map_package.xml listing them
// (smhip/map_package.h).  Like --map it is a function of the pose file as written, so --map-poses FILE builds it too -- also from the
// file --close-loops wrote.  Frames [kN, (k + 1)N) form submap k (--submap-frames N; a trailing group that is not full is dropped),
// built once on the device at --submap-voxel with local poses first^-1 * frame; its global pose is its first frame's.  The pieces'
// voxel maps take the --map-* settings.
//
// --submap-edges PATH: the submaps of the sequence and the match of every pair of consecutive ones (Submap::InsertFrame,
// builder/submap.cc:76-163; MapBuilder::SubmapPairMatch, builder/map_builder.cc:399-446).  Like --map, rank 0 works from the poses
// AS WRITTEN to the pose file once the matchers are gone.  Frames [kN, (k + 1)N) form submap k (--submap-frames N); a trailing
// group that is not full has no cloud (submap.cc:98) and is dropped.  Each submap is built on the device from its raw scans
// (smhip_submap_build_f32: local pose = first pose^-1 * pose, VoxelGrid of --submap-voxel, 0 = none) and never leaves it: it
// becomes the source against the previous submap's CalculateNormals target, then the target of the next.  IcpFast runs under
// --iterations and --early-exit.  PATH holds one line per edge: `k k+1 accepted score` and the twelve numbers of
// transform_to_next in the pose writer's format -- the match when score >= --submap-min-score, else the guess (:436-444).
#include <dirent.h>
#include <fcntl.h>
#include <signal.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdarg>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/smhip.h"
#include "../../include/smhip/kitti_scans.h"
#include "../../include/smhip/pcd.h"
#include "../../include/smhip/back_end.h"
#include "../../include/smhip/pose_graph.h"
#include "../../include/smhip/map_package.h"

namespace {

constexpr int kPoseDoubles = 18;                 // 16 column-major transform + score + iterations
using smhip::kitti::kMaxFloatsPerFile;
using smhip::kitti::ScanPrefetcher;

struct Args {
  std::string scans_dir, out_path = "kitti_pose.txt", id_file;
  unsigned long long nonce = 0;             // identifies this run's id file (launcher: pid and start time; else MASTER_PORT)
  int gpus = 1, rank = -1, world = -1, local_rank = -1;
  int batch = 256, iterations = 20, early_exit = 0, max_pairs = -1, readers = 8, matchers = 1, warmup = 1, parts = 0;
  double guess_tx = 0.0;
  bool quiet = false;
  // the static map (--map); the MRVM settings are MrvmSettings' (multi_resolution_voxel_map.h:54-65), whose defaults these are
  std::string map_path, map_poses;
  int map_every = 1, map_part_every = 0, map_points_per_cell = 10, map_max_table_log2 = 28;
  float map_resolution = 0.1f, map_threshold = 0.6f, map_hit = 0.55f, map_miss = 0.48f, map_z_offset = 0.f;
  bool map_average = false, map_rgb = false;
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
  // --gps-enu FILE: one line per scan in file order, three numbers already in ENU metres, nan = no fix (the geodetic conversion is
  // not restated); the factors' settings (isam_optimizer.h:61-66) and the antenna in the tracking frame
  std::string gps_enu;
  std::vector<std::array<double, 3>> enu;
  double gps_lever[3] = {0.0, 0.0, 0.0};
  int gps_init_num = 25, gps_sample_step = 1;
  double gps_init_angle = 1.6;
  bool gps_output_enu = false;
};

[[noreturn]] void Die(const std::string& m) { std::fprintf(stderr, "smhip_shard: %s\n", m.c_str()); std::exit(2); }

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

void Mul4(const double* a, const double* b, double* out) {              // row-major 4x4
  double r[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) { double s = 0; for (int k = 0; k < 4; ++k) s += a[4 * i + k] * b[4 * k + j]; r[4 * i + j] = s; }
  std::memcpy(out, r, sizeof(r));
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
    else if (k == "--gps-enu") a.gps_enu = val();
    else if (k == "--gps-lever") { if (std::sscanf(val().c_str(), "%lf,%lf,%lf", &a.gps_lever[0], &a.gps_lever[1], &a.gps_lever[2]) != 3) Die("--gps-lever takes x,y,z"); }
    else if (k == "--gps-init-num") a.gps_init_num = std::atoi(val().c_str());
    else if (k == "--gps-sample-step") a.gps_sample_step = std::atoi(val().c_str());
    else if (k == "--gps-init-angle") a.gps_init_angle = std::atof(val().c_str());
    else if (k == "--gps-output-enu") a.gps_output_enu = true;
    else Die("unknown argument " + k + "\nusage: smhip_shard --scans DIR [--gpus G] [--out kitti_pose.txt] [--batch 256] "
             "[--iterations 20] [--early-exit 0|1] [--guess-tx metres] [--max-pairs N] [--readers 8] [--matchers 1|2] [--warmup 1|0] [--parts 0..4]\n"
             "  static map: [--map map.pcd] [--map-poses kitti_pose.txt (map only)] [--map-every 1] [--map-part-every 0] [--map-resolution 0.1] "
             "[--map-threshold 0.6] [--map-hit 0.55] [--map-miss 0.48] [--map-points-per-cell 10] [--map-z-offset 0] [--map-average] [--map-rgb] "
             "[--map-max-table-log2 28]\n"
             "  map package: [--map-package DIR (from the poses as written, or --map-poses; submaps of --submap-frames frames at --submap-voxel, a "
             "trailing group that is not full is dropped; the pieces' maps take the --map-* settings)] [--package-piece-width 500] "
             "[--package-border-offset 100] [--package-prefix part_] [--package-descript map_package.xml]\n"
             "  submaps: [--submap-edges edges.txt] [--submap-frames 5] [--submap-voxel 0.1 (0: no voxel filter)] [--submap-min-score 0.7]\n"
             "  loop closing: [--close-loops corrected_pose.txt] [--loop-ignore-threshold 15] [--loop-detect-count 1] [--loop-history 4] "
             "[--loop-max-distance 25] [--loop-max-z 1] [--loop-use-descriptor 1] [--loop-m2dp-score 0.99] [--loop-accept-score 0.75]\n"
             "  GPS (with --close-loops): [--gps-enu enu.txt (a line per scan: east north up in metres, nan = no fix)] [--gps-lever 0,0,0] "
             "[--gps-init-num 25] [--gps-sample-step 1] [--gps-init-angle 1.6] [--gps-output-enu (the poses in the ENU frame)]");
  }
  if (a.scans_dir.empty()) Die("--scans DIR is required");
  if (!a.map_poses.empty() && a.map_path.empty() && a.map_package.empty()) Die("--map-poses needs --map PATH");
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
  if (a.gps_output_enu && a.gps_enu.empty()) Die("--gps-output-enu needs --gps-enu");
  if (!std::isfinite(a.gps_lever[0]) || !std::isfinite(a.gps_lever[1]) || !std::isfinite(a.gps_lever[2]) || !std::isfinite(a.gps_init_angle) || a.gps_init_num < 0)
    Die("bad GPS setting (--gps-lever finite, --gps-init-angle finite, --gps-init-num >= 0)");
  if (a.loop.nearest_history_pos_num < 1 || a.loop.loop_ignore_threshold < 0 || a.loop.trying_detect_loop_count < 1)
    Die("bad loop setting (--loop-history >= 1, --loop-ignore-threshold >= 0, --loop-detect-count >= 1)");
  if (a.rank < 0 && std::getenv("RANK")) a.rank = std::atoi(std::getenv("RANK"));
  if (a.world < 0 && std::getenv("WORLD_SIZE")) a.world = std::atoi(std::getenv("WORLD_SIZE"));
  if (a.local_rank < 0 && std::getenv("LOCAL_RANK")) a.local_rank = std::atoi(std::getenv("LOCAL_RANK"));
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

std::string Fmt(const char* fmt, ...) {
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

// kitti_pose.txt (map_builder.cc:626-641): 12 numbers per line, the row-major top 3x4 -> column-major 4x4.  Reading stops at the
// first line that does not hold 12 numbers.  false: the file cannot be opened.
using Pose = std::array<double, 16>;
bool ReadPoses(const std::string& path, std::vector<Pose>* poses) {
  std::ifstream f(path);
  if (!f) return false;
  std::string text;
  while (std::getline(f, text)) {
    double v[12];
    const char* p = text.c_str();
    int got = 0;
    for (; got < 12; ++got) {
      char* end = nullptr;
      v[got] = std::strtod(p, &end);
      if (end == p) break;
      p = end;
    }
    if (got < 12) break;
    Pose m{};
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m[4 * c + r] = v[4 * r + c];
    m[15] = 1.0;
    poses->push_back(m);
  }
  return true;
}

// the frames --map inserts: 0, K, 2K, ... below n_frames (--map-every K stands in for the reference's key-frame selection)
std::vector<int> MapFrames(const Args& a, int n_frames) {
  std::vector<int> v;
  for (int k = 0; k < n_frames; k += a.map_every) v.push_back(k);
  return v;
}

struct MapResult { int frames = 0, parts = 0; long long voxels = 0, points = 0; double seconds = 0.0; };

std::string MapJsonFields(const Args& a, const MapResult& m) {
  return Fmt(", \"map_file\": \"%s\", \"map_frames\": %d, \"map_voxels\": %lld, \"map_points\": %lld, \"map_parts\": %d, \"map_seconds\": %.4f, "
             "\"map_ms_per_frame\": %.3f", a.map_path.c_str(), m.frames, m.voxels, m.points, m.parts, m.seconds,
             m.frames > 0 ? 1e3 * m.seconds / m.frames : 0.0);
}

// SaveMaps (map_builder.cc:825-910) over `frames`: frame k's raw rows (intensity x 255, kitti_reader.cc:113) inserted under
// poses[k] into one device map.  --map-part-every N writes <stem>_part_<i>.pcd after every N inserted frames and starts a fresh
// map (separate_output / separate_step, :860-890, counted in frames rather than submaps); otherwise the whole map goes to --map
// PATH.  Every file has its rows in voxel-key order (SMHIP_MRVM_SORTED).  Returns 0, or 3 when the map refused a frame: the
// files of this run are then removed.  map_voxels / map_points are summed over the parts.
int BuildMap(const Args& a, const std::vector<std::string>& files, const std::vector<int>& frames, const std::vector<Pose>& poses, int device,
             MapResult* res) {
  const auto t0 = std::chrono::steady_clock::now();
  size_t max_bytes = 16;
  for (int k : frames) { struct stat sb; if (stat(files[k].c_str(), &sb) == 0) max_bytes = std::max(max_bytes, static_cast<size_t>(sb.st_size)); }
  const size_t slot_floats = std::min(kMaxFloatsPerFile, (max_bytes / 16 + 1) * 4);
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
    res->voxels += v;
    if (smhip::pcd::SaveBinary(path, n > 0 ? rows.data() : nullptr, static_cast<size_t>(n), a.map_rgb)) {
      written.push_back(path);
      res->points += n;
      ++res->parts;
    }
  };
  fresh_map();
  smhip::kitti::ScanPrefetcher scans(files, frames, a.readers, 2 * std::max(1, a.readers) + 2, /*hold_until_release=*/false, slot_floats);
  int in_part = 0, part = 0, rc = 0;
  for (size_t i = 0; i < frames.size(); ++i) {
    int n = 0, fi = -1;
    const float* rows = scans.Next(&n, &fi);
    if (!rows || fi != frames[i]) Die("map: prefetcher out of step");
    if (n < 0) Die("cannot read " + files[fi]);
    if (n == 0) {
      std::fprintf(stderr, "smhip_shard: map: %s is empty, skipped\n", files[fi].c_str());     // InsertPointCloud: "cloud is empty.", :61-64
    } else {
      const smhip_status st = smhip_mrvm_insert_transformed_f32(h, rows, 4, n, poses[fi].data(), 255.f);
      if (st != SMHIP_OK) {
        std::fprintf(stderr, "smhip_shard: map: frame %d refused: %s\n", fi, smhip_mrvm_last_error(h));
        rc = 3;
        break;
      }
      if (smhip_mrvm_last_error(h)[0]) std::fprintf(stderr, "smhip_shard: map: frame %d: %s\n", fi, smhip_mrvm_last_error(h));
    }
    ++res->frames;
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
  res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

// ---- --submap-edges -------------------------------------------------------------------------------------------------------
// inverse of an affine 4x4 (column-major), what Eigen's inverse() gives for a pose: the 3x3 block by its adjugate
Pose AffineInverse(const Pose& p) {
  auto m = [&](int r, int c) { return p[4 * c + r]; };
  const double c00 = m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1), c01 = m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2), c02 = m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0);
  const double det = m(0, 0) * c00 + m(0, 1) * c01 + m(0, 2) * c02;
  double inv[3][3] = {{c00 / det, (m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2)) / det, (m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1)) / det},
                      {c01 / det, (m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0)) / det, (m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2)) / det},
                      {c02 / det, (m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1)) / det, (m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)) / det}};
  Pose out{};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out[4 * c + r] = inv[r][c];
    out[12 + r] = -(inv[r][0] * m(0, 3) + inv[r][1] * m(1, 3) + inv[r][2] * m(2, 3));
  }
  out[15] = 1.0;
  return out;
}
Pose MulPose(const Pose& a, const Pose& b) {                              // column-major a * b
  Pose out{};
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) { double s = 0; for (int k = 0; k < 4; ++k) s += a[4 * k + r] * b[4 * c + k]; out[4 * c + r] = s; }
  return out;
}

struct SubmapResult { int submaps = 0, edges = 0, accepted = 0; double seconds = 0.0, score_sum = 0.0; };

std::string SubmapJsonFields(const Args& a, const SubmapResult& m) {
  return Fmt(", \"submap_edges_file\": \"%s\", \"submaps\": %d, \"submap_edges\": %d, \"submap_edges_accepted\": %d, \"submap_mean_score\": %.6f, "
             "\"submap_seconds\": %.4f", a.submap_edges.c_str(), m.submaps, m.edges, m.accepted, m.edges > 0 ? m.score_sum / m.edges : 0.0, m.seconds);
}

// The submaps of frames [0, n_frames) under `poses` and the match of consecutive ones; one line per edge to --submap-edges.
// Returns 0, or 3 when the device refused a submap (the file is then removed).
int BuildSubmapEdges(const Args& a, const std::vector<std::string>& files, int n_frames, const std::vector<Pose>& poses, int device, SubmapResult* res) {
  const auto t0 = std::chrono::steady_clock::now();
  const int N = a.submap_frames, S = n_frames / N;                        // a trailing group that is not full is dropped
  std::ofstream out(a.submap_edges);
  if (!out) Die("cannot write " + a.submap_edges);
  out.precision(8);
  res->submaps = S;
  if (S < 2) { res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); return 0; }
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
  const size_t slot_floats = std::min(kMaxFloatsPerFile, (max_bytes / 16 + 1) * 4);
  smhip_handle h = nullptr;
  smhip_status st = smhip_create(device, nullptr, 1, static_cast<int>(cap), static_cast<int>(cap), &h);
  if (st != SMHIP_OK) Die(std::string("smhip_create (submaps): ") + smhip_status_string(st));
  smhip_icp_options o;
  smhip_icp_default_options(&o);
  o.max_iteration = a.iterations;
  o.early_exit = a.early_exit;
  if (smhip_icp_set_options(h, &o) != SMHIP_OK) Die(smhip_last_error(h));
  // the six-decimal trip of the voxel size through the filter's text (submap.cc:148-154)
  const float voxel = a.submap_voxel > 0.f ? static_cast<float>(std::atof(std::to_string(a.submap_voxel).c_str())) : 0.f;

  std::vector<int> order(static_cast<size_t>(S) * N);
  for (size_t i = 0; i < order.size(); ++i) order[i] = static_cast<int>(i);
  smhip::kitti::ScanPrefetcher scans(files, order, a.readers, N + std::max(1, a.readers) + 2, /*hold_until_release=*/true, slot_floats);
  int rc = 0;
  for (int k = 0; k < S && rc == 0; ++k) {
    std::vector<const float*> rows(N);
    std::vector<int> n(N);
    std::vector<double> local(16 * static_cast<size_t>(N));
    const Pose first_inv = AffineInverse(poses[k * N]);
    for (int f = 0; f < N; ++f) {
      int fi = -1;
      rows[f] = scans.Next(&n[f], &fi);
      if (!rows[f] || fi != k * N + f) Die("submaps: prefetcher out of step");
      if (n[f] < 0) Die("cannot read " + files[fi]);
      const Pose lp = f == 0 ? Pose{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1} : MulPose(first_inv, poses[k * N + f]);   // submap.cc:83-87
      std::memcpy(&local[16 * static_cast<size_t>(f)], lp.data(), sizeof(double) * 16);
    }
    int m = 0;
    st = smhip_submap_build_f32(h, N, rows.data(), 4, n.data(), local.data(), voxel, &m);
    scans.ReleaseHeld();                                                  // the call returned: the rows have left the host buffers
    if (st != SMHIP_OK) { std::fprintf(stderr, "smhip_shard: submap %d refused: %s\n", k, smhip_last_error(h)); rc = 3; break; }
    if (k > 0) {
      // SubmapPairMatch(source = submap k, target = submap k - 1), map_builder.cc:399-446
      if (smhip_filter_output_to_source(h, 0) != SMHIP_OK) { std::fprintf(stderr, "smhip_shard: submap %d as source: %s\n", k, smhip_last_error(h)); rc = 3; break; }
      const Pose guess = MulPose(AffineInverse(poses[(k - 1) * N]), poses[k * N]);                  // :426-428
      double result[16], score = 0.0;
      smhip_icp_stats stats;
      st = smhip_icp_align(h, guess.data(), result, &score, &stats);
      if (st != SMHIP_OK) {                                              // no correspondence: an edge that keeps the guess
        std::fprintf(stderr, "smhip_shard: submaps %d -> %d: %s (%s)\n", k - 1, k, smhip_status_string(st), smhip_last_error(h));
        score = 0.0;
      }
      smhip::registrator::Matrix4d T;
      std::memcpy(T.data(), result, sizeof(result));
      smhip::back_end::NormalizeRotation(T);                             // :434
      const bool accepted = st == SMHIP_OK && score >= a.submap_min_score;                           // :436-444
      const double* e = accepted ? T.data() : guess.data();
      out << (k - 1) << " " << k << " " << (accepted ? 1 : 0) << " " << score;
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) out << " " << e[4 * c + r];
      out << "\n";
      ++res->edges; res->accepted += accepted ? 1 : 0; res->score_sum += score;
    }
    // the cloud is still resident: it becomes the target of the next pair (Submap::Cloud() carries normals, submap.cc:160-161)
    if (k + 1 < S && smhip_filter_output_to_target(h, 0, &m) != SMHIP_OK) {
      std::fprintf(stderr, "smhip_shard: submap %d as target: %s\n", k, smhip_last_error(h));
      rc = 3;
    }
  }
  out.close();
  smhip_destroy(h);
  if (rc != 0) std::remove(a.submap_edges.c_str());
  res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

// ---- --map-package ----------------------------------------------------------------------------------------------------------
struct PackageResult { int pieces = 0, submaps = 0; long long points = 0; double seconds = 0.0; };

std::string PackageJsonFields(const Args& a, const PackageResult& m) {
  return Fmt(", \"package_dir\": \"%s\", \"package_pieces\": %d, \"package_submaps\": %d, \"package_points\": %lld, \"package_seconds\": %.4f",
             a.map_package.c_str(), m.pieces, m.submaps, m.points, m.seconds);
}

// The submaps of frames [0, n_frames) under `poses`, each built once on the device and downloaded, then
// smhip::SaveTrajectoriesAsMapPackage over them.  The plan is made from the poses alone before any device work: a refused plan ends
// the run with 2, and so does a directory the description cannot be written into.  Returns 0, or 3 when the device refused a submap or
// an insert or a piece could not be written (this run's files are then removed).
int BuildMapPackage(const Args& a, const std::vector<std::string>& files, int n_frames, const std::vector<Pose>& poses, int device, PackageResult* res) {
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
  const size_t slot_floats = std::min(kMaxFloatsPerFile, (max_bytes / 16 + 1) * 4);
  smhip_handle h = nullptr;
  smhip_status st = smhip_create(device, nullptr, 1, static_cast<int>(cap), static_cast<int>(cap), &h);
  if (st != SMHIP_OK) Die(std::string("smhip_create (map package): ") + smhip_status_string(st) + " (is this a gfx950 GPU? there is no CPU fallback)");
  const float voxel = a.submap_voxel > 0.f ? static_cast<float>(std::atof(std::to_string(a.submap_voxel).c_str())) : 0.f;
  std::vector<smhip::MapPackageSubmap> submaps(static_cast<size_t>(S));
  int rc = 0;
  {
    std::vector<int> order(static_cast<size_t>(S) * N);
    for (size_t i = 0; i < order.size(); ++i) order[i] = static_cast<int>(i);
    smhip::kitti::ScanPrefetcher scans(files, order, a.readers, N + std::max(1, a.readers) + 2, /*hold_until_release=*/true, slot_floats);
    for (int k = 0; k < S && rc == 0; ++k) {
      std::vector<const float*> rows(N);
      std::vector<int> n(N);
      std::vector<double> local(16 * static_cast<size_t>(N));
      const Pose first_inv = AffineInverse(poses[k * N]);
      for (int f = 0; f < N; ++f) {
        int fi = -1;
        rows[f] = scans.Next(&n[f], &fi);
        if (!rows[f] || fi != k * N + f) Die("map package: prefetcher out of step");
        if (n[f] < 0) Die("cannot read " + files[fi]);
        const Pose lp = f == 0 ? Pose{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1} : MulPose(first_inv, poses[k * N + f]);   // submap.cc:83-87
        std::memcpy(&local[16 * static_cast<size_t>(f)], lp.data(), sizeof(double) * 16);
      }
      int m = 0;
      st = smhip_submap_build_f32(h, N, rows.data(), 4, n.data(), local.data(), voxel, &m);
      scans.ReleaseHeld();
      if (st != SMHIP_OK) { std::fprintf(stderr, "smhip_shard: submap %d refused: %s\n", k, smhip_last_error(h)); rc = 3; break; }
      smhip::MapPackageSubmap& sub = submaps[static_cast<size_t>(k)];
      std::memcpy(sub.global_pose.data(), poses[k * N].data(), sizeof(double) * 16);
      sub.cloud.resize(static_cast<size_t>(m));
      if (m > 0 && smhip_filter_get_output(h, &sub.cloud[0].x, nullptr, m) != SMHIP_OK) {
        std::fprintf(stderr, "smhip_shard: cloud of submap %d: %s\n", k, smhip_last_error(h)); rc = 3; break;
      }
    }
  }
  smhip_destroy(h);
  if (rc == 0) {
    smhip::MrvmSettings set;
    set.output_average = a.map_average; set.output_rgb = a.map_rgb; set.prob_threshold = a.map_threshold; set.high_resolution = a.map_resolution;
    set.hit_prob = a.map_hit; set.miss_prob = a.map_miss; set.z_offset = a.map_z_offset; set.max_point_num_in_cell = a.map_points_per_cell;
    smhip::MapPackageResult pr;
    // raw KITTI rows: intensity x 255 on the way into the map, as --map inserts them (kitti_reader.cc:113)
    if (!smhip::SaveTrajectoriesAsMapPackage(submaps, a.package, set, dir, &pr, device, 255.f, a.map_max_table_log2)) rc = 3;
    res->pieces = pr.pieces; res->submaps = pr.submaps; res->points = pr.points;
  } else {
    std::remove((dir + a.package.descript_filename).c_str());
  }
  res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

// ---- --close-loops ------------------------------------------------------------------------------------------------------------
struct LoopResult {
  int submaps = 0, loop_edges = 0, solves = 0, stop_reason = 0; double seconds = 0.0, final_cost = 0.0, moved_m = 0.0;
  int gps_factors = 0; double gps_coord[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};    // with --gps-enu; row-major
};

std::string GpsJsonFields(const Args& a, const LoopResult& m) {
  if (a.gps_enu.empty()) return "";
  std::string s = Fmt(", \"gps_factors\": %d, \"gps_coord\": [", m.gps_factors);
  for (int q = 0; q < 16; ++q) s += Fmt("%.17g%s", m.gps_coord[q], q == 15 ? "]" : ", ");
  return s;
}

std::string LoopJsonFields(const Args& a, const LoopResult& m) {
  return Fmt(", \"close_loops_file\": \"%s\", \"loop_submaps\": %d, \"loop_edges\": %d, \"pose_graph_solves\": %d, \"pose_graph_stop_reason\": %d, "
             "\"pose_graph_final_cost\": %.6g, \"loop_largest_correction_m\": %.4f, \"close_loops_seconds\": %.4f", a.close_loops.c_str(), m.submaps,
             m.loop_edges, m.solves, m.stop_reason, m.final_cost, m.moved_m, m.seconds) + GpsJsonFields(a, m);
}

// MapBuilder::ConnectAllSubmap (builder/map_builder.cc:448-613) over the submaps --submap-edges builds, from the poses as written:
// every submap is built on the device, described where it lies (M2DP), matched against the previous one (the odometry factor:
// the match when its score reaches --submap-min-score, else the guess) and handed to back_end::IsamOptimizer -- the loop detector,
// the factors, one device solve of the pose graph per update, every submap's pose written back.  A submap enters at the previous
// submap's corrected pose times its odometry factor.  After RunFinalOptimazation the frames get submap pose x local pose
// (Submap::UpdateInnerFramePose) and go to --close-loops in the pose writer's format, one line per frame of the sequence (the
// frames of a trailing group that is not full ride on the last submap), so --map-poses on that file builds the corrected map.
// Returns 0, or 3 when the device refused something (the file is then removed).
int CloseLoops(const Args& a, const std::vector<std::string>& files, int n_frames, const std::vector<Pose>& poses, int device, LoopResult* res) {
  namespace be = smhip::back_end;
  namespace bld = smhip::builder;
  using smhip::registrator::Matrix4d;
  const auto t0 = std::chrono::steady_clock::now();
  const int N = a.submap_frames, S = n_frames / N;
  res->submaps = S;
  std::ofstream out(a.close_loops);
  if (!out) Die("cannot write " + a.close_loops);
  out.precision(8);
  auto write_pose = [&out](const double* m) {                             // column-major in, the top 3 x 4 row by row out
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) out << m[4 * c + r] << ((r == 2 && c == 3) ? "\n" : " ");
  };
  if (S < 1) {
    for (int f = 0; f < n_frames; ++f) write_pose(poses[f].data());
    res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return 0;
  }
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
  const size_t slot_floats = std::min(kMaxFloatsPerFile, (max_bytes / 16 + 1) * 4);
  smhip_handle h = nullptr;
  smhip_status st = smhip_create(device, nullptr, 1, static_cast<int>(cap), static_cast<int>(cap), &h);
  if (st != SMHIP_OK) Die(std::string("smhip_create (loop closing): ") + smhip_status_string(st));
  smhip_icp_options o;
  smhip_icp_default_options(&o);
  o.max_iteration = a.iterations;
  o.early_exit = a.early_exit;
  if (smhip_icp_set_options(h, &o) != SMHIP_OK) Die(smhip_last_error(h));
  const float voxel = a.submap_voxel > 0.f ? static_cast<float>(std::atof(std::to_string(a.submap_voxel).c_str())) : 0.f;
  smhip_m2dp_options mo;
  smhip_m2dp_default_options(&mo);
  const int dlen = smhip_m2dp_length(&mo);

  be::LoopDetectorSettings settings = a.loop;
  settings.device = device;
  int rc = 0;
  {
    be::IsamOptimizerOptions io;
    io.use_gps = !a.gps_enu.empty();
    io.gps_factor_init_num = a.gps_init_num; io.gps_factor_sample_step = a.gps_sample_step; io.gps_factor_init_angle_rad = a.gps_init_angle;
    be::IsamOptimizer optimizer(io, settings, h);
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
    std::vector<int> order(static_cast<size_t>(S) * N);
    for (size_t i = 0; i < order.size(); ++i) order[i] = static_cast<int>(i);
    smhip::kitti::ScanPrefetcher scans(files, order, a.readers, N + std::max(1, a.readers) + 2, /*hold_until_release=*/true, slot_floats);
    for (int k = 0; k < S && rc == 0; ++k) {
      std::vector<const float*> rows(N);
      std::vector<int> n(N);
      std::vector<double> local(16 * static_cast<size_t>(N));
      maps.emplace_back(new bld::Submap(so));
      for (int f = 0; f < N; ++f) {
        int fi = -1;
        rows[f] = scans.Next(&n[f], &fi);
        if (!rows[f] || fi != k * N + f) Die("loop closing: prefetcher out of step");
        if (n[f] < 0) Die("cannot read " + files[fi]);
        Matrix4d P;
        std::memcpy(P.data(), poses[k * N + f].data(), sizeof(double) * 16);
        maps.back()->InsertFrame(no_points, P);
        std::memcpy(&local[16 * static_cast<size_t>(f)], maps.back()->LocalPose(f).data(), sizeof(double) * 16);   // submap.cc:83-87
      }
      int m = 0;
      st = smhip_submap_build_f32(h, N, rows.data(), 4, n.data(), local.data(), voxel, &m);
      scans.ReleaseHeld();
      if (st != SMHIP_OK) { std::fprintf(stderr, "smhip_shard: submap %d refused: %s\n", k, smhip_last_error(h)); rc = 3; break; }
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
      }
      Matrix4d from_last = Matrix4d::Identity();
      if (k > 0) {
        // SubmapPairMatch(source = submap k, target = submap k - 1), map_builder.cc:399-446, as --submap-edges does it
        if (smhip_filter_output_to_source(h, 0) != SMHIP_OK) { std::fprintf(stderr, "smhip_shard: submap %d as source: %s\n", k, smhip_last_error(h)); rc = 3; break; }
        const Pose guess = MulPose(AffineInverse(poses[(k - 1) * N]), poses[k * N]);
        double result[16], score = 0.0;
        smhip_icp_stats stats;
        st = smhip_icp_align(h, guess.data(), result, &score, &stats);
        if (st != SMHIP_OK) score = 0.0;
        Matrix4d T;
        std::memcpy(T.data(), result, sizeof(result));
        be::NormalizeRotation(T);
        if (st == SMHIP_OK && score >= a.submap_min_score) from_last = T;
        else std::memcpy(from_last.data(), guess.data(), sizeof(double) * 16);
        frame->global_pose = be::Multiply(frames.back()->global_pose, from_last);
      } else {
        frame->global_pose = maps[0]->GlobalPose();
      }
      if (k + 1 < S && smhip_filter_output_to_target(h, 0, &m) != SMHIP_OK) { std::fprintf(stderr, "smhip_shard: submap %d as target: %s\n", k, smhip_last_error(h)); rc = 3; break; }
      if (io.use_gps) {   // the fix of the submap's first frame, the frame whose pose is its global pose
        const std::array<double, 3>& e = a.enu[static_cast<size_t>(k) * N];
        if (std::isfinite(e[0]) && std::isfinite(e[1]) && std::isfinite(e[2])) {
          maps.back()->SetRelatedGpsInENU(e[0], e[1], e[2]);
          frame->has_enu = true;
          for (int c = 0; c < 3; ++c) frame->enu[c] = maps.back()->GetRelatedGpsInENU()[c];
        }
      }
      frames.push_back(frame);
      if (!optimizer.AddFrame(frame, from_last)) { std::fprintf(stderr, "smhip_shard: the pose graph could not be optimised at submap %d\n", k); rc = 3; break; }
    }
    if (rc == 0 && !optimizer.RunFinalOptimazation()) rc = 3;
    if (rc == 0) {
      res->loop_edges = optimizer.LoopEdgeCount(); res->solves = optimizer.SolveCount();
      res->stop_reason = optimizer.LastStats().stop_reason; res->final_cost = optimizer.LastStats().final_cost;
      // MapBuilder::CalculateCoordTransformToGps (map_builder.cc:748-762): with --gps-output-enu every submap pose is premultiplied
      // by the map origin's pose in the GPS frame before UpdateInnerFramePose, and the file is in the ENU frame
      const Matrix4d to_enu = optimizer.GetGpsCoordTransform();
      res->gps_factors = optimizer.GpsFactorCount();
      for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) res->gps_coord[4 * r + c] = to_enu(r, c);
      for (int k = 0; k < S; ++k) {
        maps[k]->SetGlobalPose(frames[k]->global_pose);
        maps[k]->UpdateInnerFramePose();                                   // map_builder.cc:598-601
        for (int f = 0; f < N; ++f) {
          const Matrix4d& G = maps[k]->FrameGlobalPose(f);
          const Pose& was = poses[k * N + f];
          res->moved_m = std::max(res->moved_m, std::sqrt((G(0, 3) - was[12]) * (G(0, 3) - was[12]) + (G(1, 3) - was[13]) * (G(1, 3) - was[13]) +
                                                          (G(2, 3) - was[14]) * (G(2, 3) - was[14])));
          if (!a.gps_output_enu) write_pose(G.data());
        }
        if (a.gps_output_enu) {
          maps[k]->SetGlobalPose(be::Multiply(to_enu, frames[k]->global_pose));
          maps[k]->UpdateInnerFramePose();
          for (int f = 0; f < N; ++f) write_pose(maps[k]->FrameGlobalPose(f).data());
        }
      }
      Pose last;
      std::memcpy(last.data(), (a.gps_output_enu ? be::Multiply(to_enu, frames.back()->global_pose) : frames.back()->global_pose).data(), sizeof(double) * 16);
      const Pose carry = MulPose(last, AffineInverse(poses[(S - 1) * N]));
      for (int f = S * N; f < n_frames; ++f) write_pose(MulPose(carry, poses[f]).data());
    }
  }
  out.close();
  smhip_destroy(h);
  if (rc != 0) std::remove(a.close_loops.c_str());
  res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
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
  int rc = 0;
  if (!a.map_path.empty()) {
    MapResult m;
    rc = BuildMap(a, files, frames, poses, 0, &m);
    if (rc == 0) fields += MapJsonFields(a, m);
  }
  if (rc == 0 && !a.map_package.empty()) {
    PackageResult m;
    rc = BuildMapPackage(a, files, n_frames, poses, 0, &m);
    if (rc == 0) fields += PackageJsonFields(a, m);
  }
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
  hipStream_t streams[2] = {nullptr, nullptr};
  smhip_handle hs[2] = {nullptr, nullptr};
  for (int k = 0; k < NH; ++k) HIPOK(hipStreamCreateWithFlags(&streams[k], hipStreamNonBlocking));
  hipStream_t stream = streams[0];
  // capacity: the largest scan of the directory (a KITTI scan holds at most 250 000 points: 1 000 000 floats per file are
  // read, kitti_reader.cc:93).  Slots [0, B) hold the pairs of a batch, slots [B, 2 B) park target scans that no pair of the
  // batch holds as its source already.
  size_t max_bytes = 16;
  for (const auto& f : files) { struct stat sb; if (stat(f.c_str(), &sb) == 0) max_bytes = std::max(max_bytes, static_cast<size_t>(sb.st_size)); }
  const size_t slot_floats = std::min(kMaxFloatsPerFile, (max_bytes / 16 + 1) * 4);
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
  int done = 0, my_pairs = 0;
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
    if (smhip_icp_enqueue_batch(h, nb, guesses.data()) != SMHIP_OK) Die(std::string("enqueue: ") + smhip_last_error(h));
    if (smhip_icp_export_results_device(h, nb, local_dev + static_cast<size_t>(kPoseDoubles) * base) != SMHIP_OK) Die(smhip_last_error(h));
    mark("alignments enqueued", base);
    if (turn == 0) { first_enq_s = since(t0); first_enq_pairs = nb; }
    last_enq_s = since(t0); enq_pairs += nb;
    done = base + nb;
    my_pairs += nb;
  }
  (void)done;
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
    double pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    auto write_pose = [&]() {
      for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) out << pose[4 * r + c] << ((r == 2 && c == 3) ? "\n" : " ");
    };
    write_pose();
    double score_sum = 0.0, iter_sum = 0.0;
    int bad = 0;
    for (int pair = 0; pair < n_pairs; ++pair) {
      const double* row = &all[static_cast<size_t>(kPoseDoubles) * (static_cast<size_t>(pair % world) * per + pair / world)];
      double T[16];
      for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) T[4 * r + c] = row[4 * c + r];   // column-major -> row-major
      if (!(row[17] >= 1.0)) ++bad;                                      // a pair that never ran left zeros; one that failed exports 0 iterations (smhip.h)
      Mul4(pose, T, pose);
      write_pose();
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
      if (a.map_path.empty() && a.submap_edges.empty() && a.close_loops.empty() && a.map_package.empty()) { std::printf("%s}\n", line.c_str()); line.clear(); }
    }
    if (bad) rc = 3;
  }
  (void)hipFree(local_dev); (void)hipFree(all_dev);
  for (int k = 0; k < NH; ++k) smhip_destroy(hs[k]);
  if (pinned) for (float* b : ring_buffers) (void)hipHostFree(b);
  NCCLOK(ncclCommDestroy(comm));
  for (int k = 0; k < NH; ++k) (void)hipStreamDestroy(streams[k]);
  if (rank == 0 && (!a.map_path.empty() || !a.submap_edges.empty() || !a.close_loops.empty() || !a.map_package.empty())) {
    // the static map and the submap edges from the poses as written: the pose file read back (--map-poses on that file builds
    // the same map)
    std::string fields;
    std::vector<Pose> poses;
    if (rc == 0 && (!ReadPoses(a.out_path, &poses) || static_cast<int>(poses.size()) != n_pairs + 1)) Die("cannot read back " + a.out_path);
    if (rc == 0 && !a.map_path.empty()) {
      MapResult m;
      rc = BuildMap(a, files, MapFrames(a, n_pairs + 1), poses, device, &m);
      if (rc == 0) fields += MapJsonFields(a, m);
    }
    if (rc == 0 && !a.submap_edges.empty()) {
      SubmapResult m;
      rc = BuildSubmapEdges(a, files, n_pairs + 1, poses, device, &m);
      if (rc == 0) fields += SubmapJsonFields(a, m);
    }
    if (rc == 0 && !a.close_loops.empty()) {
      LoopResult m;
      rc = CloseLoops(a, files, n_pairs + 1, poses, device, &m);
      if (rc == 0) fields += LoopJsonFields(a, m);
    }
    if (rc == 0 && !a.map_package.empty()) {
      PackageResult m;
      rc = BuildMapPackage(a, files, n_pairs + 1, poses, device, &m);
      if (rc == 0) fields += PackageJsonFields(a, m);
    }
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
