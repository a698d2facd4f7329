/* smhip.h -- C ABI of the MI355X (gfx950) scan-matching backend.
 *
 * This is the drop-in boundary for StaticMapping's per-frame registration hot
 * path.  Nothing like it exists in the reference: the reference
 * reaches its registrators through the C++ class
 *   static_map::registrator::Interface      /root/reference/registrators/interface.h:67-116
 * created by
 *   CreateMatcher(const MatcherOptions&)    /root/reference/registrators/interface.cc:139-173
 * The C++ mirror of that class lives in include/smhip/registrator.h and is a
 * thin adapter over the entry points below; INTEGRATION.md shows the lines a
 * maintainer adds to interface.cc to select it.
 *
 * Conventions
 *   - plain C types only; no exceptions cross the boundary; every call returns
 *     an smhip_status (0 = ok) and smhip_last_error(h) gives the text;
 *   - 4x4 transforms are COLUMN-major doubles (Eigen::Matrix4d storage), and
 *     map SOURCE-frame points into the TARGET frame
 *     (pose_source = pose_target * align_result, builder/map_builder.cc:354);
 *   - a handle owns one HIP stream (or borrows the caller's), all its device
 *     buffers and a fixed number of independent "pair slots"; slot 0 is what the
 *     single-pair registrator::Interface adapter uses, slots 0..B-1 are used by
 *     the batched / sharded benchmark path.  One thread per handle; different
 *     handles are independent (the reference runs up to 6 matchers
 *     concurrently, builder/map_builder.cc:655,706-708).
 */
#ifndef SMHIP_H_
#define SMHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int smhip_status;
enum {
  SMHIP_OK = 0,
  SMHIP_ERR_INVALID_ARGUMENT = 1,
  SMHIP_ERR_NO_DEVICE = 2,      /* no gfx950 device / HIP runtime failure at create */
  SMHIP_ERR_HIP = 3,            /* a HIP call failed; see smhip_last_error */
  SMHIP_ERR_NOT_READY = 4,      /* Align before SetInputSource/SetInputTarget */
  SMHIP_ERR_NO_NORMALS = 5,     /* IcpFast target without normals (icp_fast.cc:430 CHECK) */
  SMHIP_ERR_NO_MATCH = 6,       /* no finite correspondence (icp_fast.cc:81 CHECK(!values.empty())) */
  SMHIP_ERR_CAPACITY = 7        /* cloud larger than the handle was created for */
};

typedef struct smhip_context* smhip_handle;

/* nn_mode values */
enum {
  SMHIP_NN_BRUTE = 0,           /* LDS-tiled exact brute force (BASELINE config #2) */
  SMHIP_NN_GRID = 1,            /* bit-rank voxel grid, exact with brute-force fallback */
  SMHIP_NN_NABO = 2             /* the reference's own search: libnabo 1.0.7's KDTREE_LINEAR_HEAP tree rebuilt per Align and
                                   its epsilon-approximate knn (icp_fast.cc:169-180, 464-467), nn_epsilon = 3.16 there.
                                   APPROXIMATE by design: the mode that reproduces what a libnabo build of the reference
                                   returns; the exact modes differ from it by millimetres */
};

/* Options of the IcpFast-equivalent matcher.  max_iteration / dist_outlier_ratio
 * mirror IcpFast::options_ (/root/reference/registrators/icp_fast.h:56-60) and
 * are the names registered at icp_fast.cc:407-419. */
typedef struct smhip_icp_options {
  int32_t max_iteration;        /* default 100 */
  float dist_outlier_ratio;     /* default 0.7f */
  int32_t early_exit;           /* 1 = CheckConvergence enabled (reference behaviour, icp_fast.cc:377-405);
                                   0 = run exactly max_iteration iterations (throughput runs) */
  int32_t nn_mode;              /* SMHIP_NN_GRID (default), SMHIP_NN_BRUTE or SMHIP_NN_NABO */
  float grid_cell;              /* voxel edge in metres for SMHIP_NN_GRID (default 0.25) */
  int32_t grid_max_ring;        /* largest ring searched in the grid before the brute-force fallback (default 8: rings 1, 2, 4, 8) */
  int32_t check_every;          /* host polls the device "all done" word every this many iterations (default 8) */
  int32_t use_ball;             /* 1 (default): ball-bounded search seeded by the previous iteration's match, with
                                   certified trimming (matches beyond the quantile carry a proven lower bound
                                   instead of an exact distance); 0: exact ring search for every query */
  int32_t exact_matches;        /* 1: refine every lower bound to the exact match in every iteration (default 0;
                                   the transform / score are identical either way, only rejected matches differ) */
  float ball_radius;            /* largest search radius of the ball search in metres (default 0.3; queries with nothing that close
                                   are lower-bounded and, if the trimming quantile reaches the bound, refined exactly) */
  float ball_cap_factor;        /* next iteration's search-radius cap = factor x this iteration's quantile distance (default 1.5) */
  int32_t no_certify;           /* 1 = search every query in every iteration instead of first trying the nearest-neighbour
                                   certificate (runner-up bound minus the query's motion); default 0 = certificates on */
  int32_t no_lds_table;         /* 1: voxel lookups from global memory (nn_ball) instead of LDS row tables (nn_ball_lds) */
  int32_t no_overlap;           /* 1: keep a batch on one stream (default 0: a batch is split into parts of >= 16 pairs on
                                   separate streams so one part's latency-bound launches hide behind the others' NN) */
  int32_t overlap_streams;      /* number of such parts, 1..4; 0 = default (2; 4 is 1.5-5 % faster on 512-pair batches, slower on 256-pair ones).
                                 * More than 2 parts (or RCCL beside the matcher) need more hardware queues than the runtime's default 4, or two
                                 * parts share a queue and run one after the other: export GPU_MAX_HW_QUEUES=8 before the process's first HIP
                                 * call (smhip_shard and bench.py do) */
  int32_t split_after;          /* batches: iterations >= this run the certificate pass and the search of the failing queries as two
                                   launches instead of the fused kernel (pays once few certificates fail).  0 = automatic: 2 for a
                                   handle's first batch, then the first iteration in which the median pair of the PREVIOUS batch
                                   searched fewer than a fifth of its queries (smhip_icp_profile.split_after_used reports it);
                                   negative = never.  Results are identical either way. */
  float nn_epsilon;             /* SMHIP_NN_NABO only: libnabo's epsilon (default 3.16, icp_fast.cc:174; 0 = exact through the tree) */
  int32_t no_fused_sums;        /* batches: 1 = certificate pass and normal-equation sums as two passes over the source in every iteration.
                                   Default 0: from split_after on ONE pass does both, summing the matches below a predicted band of
                                   histogram bins around the trimming quantile and leaving the band's members for the exact select
                                   (a missed prediction costs that pair one plain pass).  The same matches, distances and kept set
                                   either way; the 29 sums are added in a different (fixed) order: poses agree to ~1e-12.
                                   SMHIP_NN_NABO has the same form (traversal certificates instead of distance bounds), from the
                                   iteration on in which the previous batch's median pair walked fewer than a fifth of its queries. */
  int32_t no_single_kernel;     /* a single pair (smhip_icp_align) or a batch of up to 8 pairs: 1 = the iteration loop as separate launches per
                                   iteration.  Default 0: the whole loop of icp_fast.cc:484-523 and the score as ONE cooperative launch whose
                                   workgroups stay resident and meet at grid barriers, a row of the grid per pair (exact-search mode with
                                   certificates; other modes and clouds of more than 16 rounds of 256 points per resident workgroup take the
                                   separate launches).  The same matches, distances and kept sets either way; the sums are added in a different
                                   (fixed) order: poses agree to ~1e-14.  Cooperative launches of several handles run one after the other. */
} smhip_icp_options;

/* Per-call statistics (all optional to read). */
typedef struct smhip_icp_stats {
  int32_t iterations;           /* iterations executed by this pair */
  int32_t kept;                 /* correspondences kept by the trimmed-distance filter in the last iteration */
  double limit_d2;              /* the quantile (squared distance) of the last iteration */
  int32_t fallback_queries;     /* queries resolved by the brute-force fallback, summed over iterations */
  int32_t status;               /* per-pair smhip_status */
  int32_t hard_queries;         /* matches recorded as lower bounds by the ball search, summed over iterations */
  int32_t refined_iterations;   /* iterations in which those bounds had to be refined to exact matches */
  int32_t searched_queries;     /* queries that needed a search (certificate failed / first iteration), summed over iterations */
  int32_t fused_iterations;     /* iterations whose sums came from the fused certificate pass (its quantile band held) */
} smhip_icp_stats;

/* Kernel-time breakdown collected when profiling is enabled (HIP events around
 * every launch, recorded on the stream the launch goes to: a batch of >= 16 pairs
 * runs as two halves on two streams, so the sums can exceed the wall time).  Names follow the reference's
 * REGISTER_BLOCK labels where one exists (icp_fast.cc:103,171,261,484). */
typedef struct smhip_icp_profile {
  double ms_prepare;            /* target centring + grid build (replaces kd-tree build, icp_fast.cc:464-467) */
  double ms_find_closests;      /* "FindClosests": all NN kernels (main + fallback), summed over launches */
  double ms_error_elements;     /* "ErrorElements"+"ComputePointToPlane" accumulate kernel */
  double ms_solve;              /* select + 6x6 solve + convergence kernel */
  int32_t launches_find_closests;
  int32_t launches_error_elements;
  int32_t launches_solve;
  int32_t launches_nn_main;     /* launches of the dominant NN kernel alone (nn_ball_lds; the certificate / listed-search
                                   launches of the converged iterations count under find_closests only) */
  double ms_nn_main;            /* its summed duration (subset of ms_find_closests) */
  double pairs_nn_main;         /* pairs those launches covered, summed (pairs per launch = this / launches_nn_main) */
  double ms_nn_certify;         /* the certificate pass (nn_certify) alone: summed duration (subset of ms_find_closests) */
  double pairs_nn_certify;      /* pairs its launches covered, summed */
  int32_t launches_nn_certify;
  int32_t split_after_used;     /* iteration from which the last batched enqueue ran certificate pass + listed search (filled with or
                                   without profiling; 0 = the last enqueue was not a batch of >= 16 pairs) */
  double ms_nn_listed;          /* the search of the queries whose certificate failed (nn_ball_listed; SMHIP_NN_NABO: the list walk) */
  double pairs_nn_listed;
  double ms_nn_refine;          /* the refinement launches of an iteration (nn_validate + nn_ring + nn_fallback), near-empty when the
                                   quantile stays below every recorded lower bound */
  double pairs_error_elements;  /* pairs the accumulate launches covered, summed */
  int32_t launches_nn_listed;
  int32_t launches_nn_refine;
} smhip_icp_profile;

/* ---- library / device ------------------------------------------------- */
int smhip_version(void);
const char* smhip_status_string(smhip_status s);
/* number of visible HIP devices whose gcnArchName starts with "gfx950"; <0 on runtime failure */
int smhip_device_count(void);

/* ---- handle ------------------------------------------------------------ */
/* stream: a hipStream_t to borrow (e.g. torch's current stream) or NULL to own one.
 * pair_slots >= 1; max_source_points / max_target_points size the device arena once (max_source_points <= 4194304).
 * (no hipMalloc happens inside Align). */
smhip_status smhip_create(int device, void* stream, int pair_slots, int max_source_points,
                          int max_target_points, smhip_handle* out);
smhip_status smhip_destroy(smhip_handle h);
const char* smhip_last_error(smhip_handle h);
void smhip_icp_default_options(smhip_icp_options* o);
smhip_status smhip_icp_set_options(smhip_handle h, const smhip_icp_options* o);
smhip_status smhip_synchronize(smhip_handle h);

/* ---- inputs (host memory; copied to the device immediately) ------------
 * replaces IcpFast::SetInputSource / SetInputTarget (icp_fast.cc:421-453), which
 * deep-copy the caller's EigenPointCloud (3xN column-major f64 = xyzxyz...). */
smhip_status smhip_set_source_f64(smhip_handle h, int slot, const double* xyz_colmajor_3xN, int n);
smhip_status smhip_set_target_f64(smhip_handle h, int slot, const double* xyz_colmajor_3xN,
                                  const double* normals_colmajor_3xN, int n);
/* The source is re-ordered along a Morton curve on upload (spatially coherent wavefronts); ids / d2
 * returned by smhip_icp_get_matches are in the CALLER's order again.
 * float32 points with a stride in floats: stride 4 = KITTI .bin rows (ros_node/kitti_reader.cc:91-121),
 * stride 5 = data::InnerPointType AoS {x,y,z,intensity,factor} (builder/data/cloud_types.h:46-56). */
smhip_status smhip_set_source_f32(smhip_handle h, int slot, const float* xyz, int stride_floats, int n);
/* `count` source clouds at once (the sequence driver's batch: SetInputSource of many pairs): cloud k = rows[k], n[k] rows of 4
 * floats (KITTI rows) into slots[k].  One host-to-device copy per cloud, ONE Morton ordering for the batch (a single upload
 * costs ~25 small launches).  rows[k] in pinned memory (hipHostMalloc / hipHostRegister) are copied from where they lie,
 * asynchronously: they must stay untouched until the handle's stream has passed the copies (smhip_synchronize, or any call
 * that blocks on the stream, e.g. smhip_prepare_targets_from_sources); pageable rows go through the handle's staging buffer
 * one cloud at a time.  Needs stride 4. */
smhip_status smhip_set_sources_f32_batch(smhip_handle h, int count, const int* slots, const float* const* rows, const int* n);
/* allocates the workspaces of the batched calls (smhip_set_sources_f32_batch, smhip_prepare_targets_from_sources) now rather
 * than inside the first batch -- several GB for a handle of hundreds of slots */
smhip_status smhip_reserve_batch_workspaces(smhip_handle h);
smhip_status smhip_set_target_f32(smhip_handle h, int slot, const float* xyz, int xyz_stride_floats,
                                  const float* normals, int normals_stride_floats, int n);
/* Re-use slot `from`'s device-resident clouds in slot `to` (benchmark replication; no host copy). */
smhip_status smhip_copy_slot(smhip_handle h, int from, int to);

/* ---- IcpFast::Align (icp_fast.cc:455-529) ------------------------------
 * Aligns slots [0, npairs).  guesses/results: npairs * 16 doubles, column-major.
 * scores: exp(-mean sqrt(d2)) over kept matches of the last iteration (icp_fast.cc:518-521).
 * stats may be NULL.  Blocking: returns after the results are in host memory. */
smhip_status smhip_icp_align(smhip_handle h, const double guess[16], double result[16], double* score,
                             smhip_icp_stats* stats);
smhip_status smhip_icp_align_batch(smhip_handle h, int npairs, const double* guesses, double* results,
                                   double* scores, smhip_icp_stats* stats);
/* The same for the pair slots [first_slot, first_slot + npairs): lets one handle keep several independent jobs resident
 * (the back end's concurrent SubmapPairMatch tasks, builder/map_builder.cc:655; an ICP pair beside its score pair). */
smhip_status smhip_icp_align_range(smhip_handle h, int first_slot, int npairs, const double* guesses, double* results,
                                   double* scores, smhip_icp_stats* stats);
/* IcpUsingPointMatcher::Align's post-hoc score (icp_pointmatcher.cc:112-143): one FindClosests + TrimmedDist(ratio) pass of
 * the slot's source moved by T (column-major) against the slot's target; *score = exp(-mean distance of the kept matches),
 * *kept (may be NULL) = their number.  The target needs no normals. */
smhip_status smhip_icp_trimmed_score(smhip_handle h, int slot, const double T[16], float dist_outlier_ratio, double* score,
                                     int32_t* kept);
/* The 6x6 information of an alignment at T (column-major, source -> target), in the tangent convention of the pose graph's
 * BETWEEN residual below (rotation first, T <- T * [Exp(phi), rho]).  The matches are those of ONE FindClosests pass at T, every
 * one exact; the kept set is TrimmedDist(ratio)'s over them, the rule and the int(n * ratio) rank of smhip_icp_trimmed_score:
 * kept = d2 finite and d2 <= limit_d2.  For a kept source point s (caller's coordinates) matched to target q with normal n:
 * m = R^T n, r = n . (R s + t - q), J = [s x m ; m].  H = sum J J^T (row-major, symmetric), sum_r2 = sum r^2, n_finite = the
 * matches with finite d2.  All sums are f64 from the stored f32 values, added in an order fixed by the cloud's size alone: two
 * calls, the range call and the single calls, and either launch form of the matching pass give the same bits.  Needs a target
 * with normals (SMHIP_ERR_NO_NORMALS).  The caller's ICP options are unchanged afterwards.  A pair without a finite
 * correspondence has its status in out[k].status and H = 0; the call then returns the first such status, as the align calls do. */
typedef struct smhip_icp_information {
  double H[36];
  double sum_r2;
  double limit_d2;
  int32_t kept, n_finite;
  int32_t status, reserved;
} smhip_icp_information;
smhip_status smhip_icp_information_at(smhip_handle h, int slot, const double T[16], float dist_outlier_ratio,
                                      smhip_icp_information* out);
smhip_status smhip_icp_information_range(smhip_handle h, int first_slot, int npairs, const double* Ts, float dist_outlier_ratio,
                                         smhip_icp_information* out);
/* Asynchronous halves of the batch call: enqueue leaves everything on the stream (needs
 * early_exit = 0 or accepts running all max_iteration launches), fetch blocks and copies out. */
smhip_status smhip_icp_enqueue_batch(smhip_handle h, int npairs, const double* guesses);
smhip_status smhip_icp_fetch_batch(smhip_handle h, int npairs, double* results, double* scores,
                                   smhip_icp_stats* stats);

/* Device-resident copy of the last results: writes npairs * 18 doubles to device memory at
 * dev_out (16 column-major transform + score + iterations) on the handle's stream, so a collective
 * (RCCL gather of the poses) can consume them without a host round trip.
 * The row has no status column: a pair that smhip_icp_fetch_batch would answer with a status other than
 * SMHIP_OK (no finite correspondence -- also when it was lost after the first iteration --, a non-finite target,
 * a single launch that stopped itself) exports iterations = 0 whatever count it reached, with the transform and
 * score it was left with (the guess and 0 for "no finite correspondence").  Every finished pair exports
 * iterations >= 1, so `row[17] >= 1` is the test for "this pair has a result". */
smhip_status smhip_icp_export_results_device(smhip_handle h, int npairs, void* dev_out);

/* ---- target preparation (host) -------------------------------------------
 * EigenPointCloud::CalculateNormals (builder/data/cloud_types.cc:347-368): kd-box subsampling +
 * unconstrained-LS normals.  The reference's CALLER runs it before SetInputTarget
 * (builder/map_builder.cc:286,389), so it is a free function, not part of Align.
 * xyz: 3xN column-major; outputs need room for n points; *n_out = surviving points. */
smhip_status smhip_calculate_normals_f64(const double* xyz_colmajor_3xN, int n, double* out_xyz,
                                         double* out_normals, int* n_out);

/* Device-side target preparation: upload a raw scan (float32 rows, stride in
 * floats) and run CalculateNormals on the GPU; the surviving points + normals become `slot`'s target.
 * *n_out = number of target points.  smhip_prepare_target_from_source does the same from the source
 * cloud already resident in slot `from` (scan-to-scan sequences: scan i is the source of pair i-1 and the
 * target of pair i, uploaded once). */
smhip_status smhip_prepare_target_f32(smhip_handle h, int slot, const float* xyz, int stride_floats, int n, int* n_out);
smhip_status smhip_prepare_target_from_source(smhip_handle h, int from_slot, int to_slot, int* n_out);
/* Batched form: count targets in ONE pass (one kd forest, one sort per tree level for all scans);
 * target of to_slots[k] = CalculateNormals(source cloud of from_slots[k]); n_out[k] = its size. */
smhip_status smhip_prepare_targets_from_sources(smhip_handle h, int count, const int* from_slots, const int* to_slots, int* n_out);

/* CalculateNormals of the RAW target resident in from_slot becomes the (points + normals) target of to_slot -- the
 * reference filter of the IcpUsingPointMatcher chain (SamplingSurfaceNormal, icp_pointmatcher.cc:176-184) without a
 * second upload of the reference cloud.  from_slot != to_slot. */
smhip_status smhip_prepare_target_from_target(smhip_handle h, int from_slot, int to_slot, int* n_out);
/* RandomSamplingDataPointsFilter (icp_pointmatcher.cc:170-174) on the device: the source of to_slot = the points of
 * from_slot's source whose uniform draw is < prob (prob >= 1 keeps everything).  The draw is a pure function of
 * (seed, the point's index in the cloud as uploaded): splitmix64(seed << 32 | index) >> 11, times 2^-53. */
smhip_status smhip_sample_source(smhip_handle h, int from_slot, int to_slot, float prob, uint32_t seed, int* n_out);
/* Target-side structures (the ICP search grid, the NDT voxel table; for NdtWithGicp also the down-sampled target, the
 * correspondence grid and the target's GICP covariances) are pure functions of the target cloud and the options;
 * single-pair calls keep them while a slot's target is unchanged -- the front end aligns scan after scan against one key
 * frame / submap (builder/map_builder.cc:379-392) -- and rebuild them whenever the target is set, prepared or copied again
 * or an option they depend on changes.  enable = 0: nothing survives from one Align to the next, as in the reference
 * (icp_fast.cc:464-467, ndt.cc:54, ndt_gicp.cc:55-81); default 1.  Results are identical either way. */
smhip_status smhip_set_target_cache(smhip_handle h, int enable);
/* IcpFast Aligns of up to 8 pairs run as ONE cooperative launch (csrc/icp_one.hip: the loop of icp_fast.cc:484-523 + the score).
 * Should that launch stop itself (its barrier watchdog, its workgroups' consistency columns, a score whose count differs from the
 * kept count), the fetch runs the Align again as separate launches and the handle keeps to them: *launches_used = Aligns that went
 * through the one launch, *fallbacks = how often that happened (0 on every run recorded so far).  Either pointer may be NULL. */
smhip_status smhip_icp_single_launch_counts(smhip_handle h, int64_t* launches_used, int64_t* fallbacks);
/* With split_after = 0 a batch of >= 16 pairs switches from the every-query search to certificates + listed search at the iteration
 * the PREVIOUS batch suggests (a front end's guesses are alike from call to call); results never depend on it, only the time.  This
 * call forgets what earlier batches taught the handle -- e.g. after a warm-up batch of made-up clouds (smhip_shard) -- so that the
 * next batch starts from the defaults a new handle has. */
smhip_status smhip_icp_forget_search_history(smhip_handle h);
/* Inner motion compensation: de-skew of the source inside every IcpFast iteration (registrator::Interface::EnableInnerCompensation).
 * The reference's branch for it (icp_fast.cc:486-491 -> cloud_types.cc:306-321) is undefined behaviour as written, so what runs is
 * DEFINED HERE (tests/icp_compensation_ref.py is the text): a continuous-time point-to-plane ICP in which the guess is the pose at
 * the start of the sweep, the motion during the sweep is the unknown and the result is the pose at its end.  With n rows uploaded
 * and i the CALLER's row index, f_i = (double) i / n; in every iteration
 *     P_i = R((double)(float) f_i) * (T(-mu) guess s_i) + T_iter.t * (double)(float) f_i
 * with R Eigen's slerp from the identity to T_iter's rotation (not normalised), and EACH COORDINATE OF P_i IS ROUNDED TO FLOAT: the
 * step cloud is a float cloud, which is what the search kernels stream.  The normal equations are A = sum f_i^2 J_i J_i^T and
 * b = -sum f_i J_i r_i with the unrounded f_i.  Search, quantile, solve, T_iter = dT * T_iter, CheckConvergence, the score and
 * result = T(mu) T_iter T(-mu) guess are those of the rigid Align.
 * enable != 0 allocates the step cloud's array for every slot of the handle (12 bytes per source point; nothing is allocated
 * inside an Align) and makes every form of Align -- single, batch, range, enqueue / fetch / export -- run the mode; 0 (default)
 * puts the rigid Align back, bit for bit.  The mode searches every query in every iteration (certificates assume a rigid step) and
 * runs with nn_mode SMHIP_NN_GRID only: an Align under another nn_mode returns SMHIP_ERR_INVALID_ARGUMENT before anything is
 * touched.  smhip_icp_find_closests, smhip_icp_trimmed_score and smhip_icp_information_* stay rigid passes. */
smhip_status smhip_icp_set_inner_compensation(smhip_handle h, int enable);
smhip_status smhip_icp_get_inner_compensation(smhip_handle h, int* enabled);
/* what the handle was created with / what a slot currently holds (any pointer may be NULL) */
smhip_status smhip_get_capacity(smhip_handle h, int* pair_slots, int* max_source_points, int* max_target_points);
smhip_status smhip_get_cloud_sizes(smhip_handle h, int slot, int* n_source, int* n_target, int* has_normals);

/* ---- introspection for parity tests ------------------------------------
 * Matches of the LAST executed iteration of `slot` (FindClosests output, icp_fast.cc:169-180):
 * ids index the target cloud in the caller's order, d2 are squared distances (float32).  Every match
 * the trimmed-distance filter KEPT is exact; with use_ball = 1 and exact_matches = 0 a rejected match
 * may carry a certified lower bound (> the quantile) and the best target seen so far instead. */
smhip_status smhip_icp_get_matches(smhip_handle h, int slot, int32_t* ids, float* d2, int n);
/* Debugging / tests: the search grid resident in `slot` (the structure the last Align or find_closests on it built or kept), copied
 * to host buffers after a synchronisation.  mu[3]: the target mean; cell_origin[4]: the cell edge h, then the grid's origin x y z
 * (centred coordinates); dims[7]: nx, ny, nz, wx (32-cell words per row), nw (words), nocc (occupied cells), nt (points).
 * words: nw pairs {occupancy bits, exclusive rank of the word's first cell}; cstart: nocc + 1 run starts of the cell-sorted target;
 * tq / tn: nt rows of 4 floats -- the centred point with the caller's index as the bits of w, and its normal with w = 0 -- cells in
 * linear order, a cell's points by caller index.  Any of the four may be NULL; a capacity (in words, entries, rows) below what
 * the structure holds -- SMHIP_ERR_CAPACITY with the geometry already written; no grid in the slot -- SMHIP_ERR_NOT_READY. */
smhip_status smhip_icp_debug_get_grid(smhip_handle h, int slot, double mu[3], float cell_origin[4], int32_t dims[7],
                                      uint32_t* words, int words_cap, uint32_t* cstart, int cstart_cap, float* tq, float* tn, int points_cap);
/* Debugging / tests: the libnabo kd-tree resident in `slot` (nn_mode = SMHIP_NN_NABO: the structure the last Align or find_closests
 * on it built or kept), copied to host buffers after a synchronisation.  mu[3]: the target mean; max_error2: (1 + nn_epsilon)^2, the
 * float the search multiplies by; dims[4]: node count, nt (points), leaf blocks, ns (source points).  nodes: pairs of words -- inner
 * node {cut value bits, (left child << 2) | cut dimension}, the right child behind the left one; leaf {first, (count << 2) | 3}.
 * tq: nt rows of 4 floats, the centred point with the caller's index as the bits of w, in final bucket order.  leaf: blocks of 24
 * floats x[8] y[8] z[8], the bucket that starts at tq position `first` in block first >> 2, unused entries +inf (blocks no bucket
 * starts in are unspecified).  work / lb: per source point in the CALLER's order, the buckets its last walk scanned (saturating at
 * 255) and the stored certificate word (the slack plus the pair's motion potential at the time of the walk).  work / lb are
 * meaningful only for the source the slot's last find_closests / Align in this mode walked: after a new source was set, or before
 * any such call, they are whatever the arrays hold, returned with SMHIP_OK -- the caller sees to the order.  Any pointer may be
 * NULL; a capacity (in nodes, rows, blocks, queries) below what the structure holds -- SMHIP_ERR_CAPACITY with mu, max_error2 and
 * dims already written; no kd-tree in the slot -- SMHIP_ERR_NOT_READY.  Changes no state. */
smhip_status smhip_icp_debug_get_kd_tree(smhip_handle h, int slot, double mu[3], float* max_error2, int32_t dims[4],
                                         uint32_t* nodes, int nodes_cap, float* tq, int points_cap, float* leaf, int leaf_cap,
                                         uint8_t* work, float* lb, int queries_cap);
/* One FindClosests pass only: transform the slot's source by T (column-major 4x4, applied AFTER
 * centring exactly as Align does) and return ids / d2 without running ICP. */
smhip_status smhip_icp_find_closests(smhip_handle h, int slot, const double T[16], int32_t* ids, float* d2, int n);

/* ---- registrators::Ndt (pclomp NDT, /root/reference/registrators/ndt.cc:29-64) -------------------
 * Uses slot 0's clouds (upload them with smhip_set_source_f32 / smhip_set_target_f32: the reference's
 * Ndt converts the InnerPointType AoS to pcl::PointXYZ, ndt.cc:44-51; the target needs no normals).
 * Defaults are the wrapper's: resolution 1.0 (ndt.cc:31), KDTREE neighbourhood (ndt.cc:33), step 0.1,
 * outlier ratio 0.55, transformation epsilon 0.1, 35 iterations (pclomp/ndt_omp_impl.hpp:47-76).
 *
 * search_method is pclomp's setNeighborhoodSearchMethod with the enum's own values (pclomp/ndt_omp.h:52-57): which voxels a
 * transformed point is paired with in computeDerivatives (ndt_omp_impl.hpp:233-247).  KDTREE: the voxels whose centroid lies
 * within `resolution` of the point.  The direct rules (voxel_grid_covariance_omp_impl.hpp:373-442) start from the cell
 * floor(x / resolution) -- a float division -- and keep each cell of their stencil that lies inside the target's voxel box, is
 * occupied and holds min_points_per_voxel points, whatever the distance: DIRECT1 the cell itself, DIRECT7 the cell and its
 * six face neighbours (pclomp's own default, ndt_omp_impl.hpp:74), DIRECT26 the 26 cells around it WITHOUT the cell itself.
 * That last stencil is pcl::getAllNeighborCellIndices() of PCL 1.8.1, which the reference does not vendor: like the rest of
 * the registrator restatements it is unpinned.  The rule applies to smhip_ndt_align, smhip_ndt_align_batch,
 * smhip_ndt_compute_derivatives[_ex] and smhip_ndt_time_derivatives; the voxel table does not depend on it (a kept table is
 * reused when only the rule changes), and NdtWithGicp's NDT stage (stock PCL, which has no such switch) never uses it. */
#define SMHIP_NDT_SEARCH_KDTREE 0
#define SMHIP_NDT_SEARCH_DIRECT26 1
#define SMHIP_NDT_SEARCH_DIRECT7 2
#define SMHIP_NDT_SEARCH_DIRECT1 3
typedef struct smhip_ndt_options {
  float resolution;
  float step_size;
  float outlier_ratio;
  float transformation_epsilon;
  int32_t max_iterations;
  int32_t min_points_per_voxel;      /* voxel_grid_covariance_omp.h:204 */
  float min_covar_eigvalue_mult;     /* voxel_grid_covariance_omp.h:205 */
  int32_t search_method;             /* SMHIP_NDT_SEARCH_*; 0 = KDTREE; anything else is refused by smhip_ndt_set_options */
  int32_t reserved[4];
} smhip_ndt_options;

typedef struct smhip_ndt_stats {
  int32_t iterations;                /* nr_iterations_ */
  int32_t derivative_calls;          /* computeDerivatives evaluations (1 + one per Newton iteration) */
  int32_t voxels;                    /* occupied voxels of the target */
  int32_t status;
  double trans_probability;          /* score / N (ndt_omp_impl.hpp:170) */
  double pairs_last;                 /* (point, voxel) pairs of the last evaluation = N * mean neighbours */
} smhip_ndt_stats;

void smhip_ndt_default_options(smhip_ndt_options* o);
smhip_status smhip_ndt_set_options(smhip_handle h, const smhip_ndt_options* o);
/* Ndt::Align: voxel grid build + Newton iterations + getFitnessScore.  *score = mean squared 1-NN
 * distance of the aligned source to the raw target (LOWER is better, unlike the ICP score). */
smhip_status smhip_ndt_align(smhip_handle h, const double guess[16], double result[16], double* score,
                             smhip_ndt_stats* stats);
/* npairs independent Ndt::Align calls -- pair slots first_slot .. first_slot + npairs - 1, clouds set with smhip_set_source_f32 /
 * smhip_set_target_f32 on those slots -- advanced in lock-step: the back end runs up to six SubmapPairMatch tasks at once with
 * whichever matcher is configured (builder/map_builder.cc:399-446, 655).  Every pair's Newton / More-Thuente state machine
 * (pclomp/ndt_omp_impl.hpp:81-171, 757-916) lives in device memory and asks for the evaluations the reference would make, in the
 * reference's order; a round = one computeDerivatives launch over all pairs still running + one control launch (fold, 6x6 solve,
 * line-search decision, next pose), the voxel tables are built in one pass and the fitness scores in another: the whole batch is one
 * submission and one synchronise.  Results are the single calls' bit for bit.
 * guesses / results: npairs column-major 4x4; scores / stats: npairs entries (may be NULL). */
smhip_status smhip_ndt_align_batch(smhip_handle h, int first_slot, int npairs, const double* guesses, double* results,
                                   double* scores, smhip_ndt_stats* stats);
/* parity-test hooks: VoxelGridCovariance::applyFilter output and one computeDerivatives evaluation
 * at pose6 = (tx, ty, tz, rx, ry, rz).  icovs hold xx xy xz yy yz zz as float; hess is row-major 6x6. */
smhip_status smhip_ndt_build_voxels(smhip_handle h, int* n_voxels);
smhip_status smhip_ndt_get_voxels(smhip_handle h, int capacity, int32_t* keys, int32_t* counts, double* means,
                                  float* icovs, float* centroids);
/* copy slot's current target (as uploaded / prepared) back to the host: xyz and normals, 3 floats each */
smhip_status smhip_get_target_f32(smhip_handle h, int slot, float* xyz, float* normals, int n);
/* copy slot's resident source back to the host in the order the device holds it (Morton order after smhip_set_source_f32 /
 * smhip_set_sources_f32_batch): 4 floats per row, x y z and in .w the bits of the row's index in the cloud the caller uploaded.
 * That order is the point index of the CalculateNormals calls that build from a source slot. */
smhip_status smhip_get_source_f32(smhip_handle h, int slot, float* xyzw, int n);
smhip_status smhip_ndt_compute_derivatives(smhip_handle h, const double pose6[6], int compute_hessian,
                                           double* score, double grad[6], double hess[36]);
/* the same evaluation in either arithmetic -- double_math = 0: pclomp's float per-pair math (Ndt), 1: stock PCL's double
 * (the NDT stage of NdtWithGicp) -- for this call only, and with the number of (point, voxel) pairs that entered the sums
 * (pairs may be NULL). */
smhip_status smhip_ndt_compute_derivatives_ex(smhip_handle h, const double pose6[6], int compute_hessian, int double_math,
                                              double* score, double grad[6], double hess[36], double* pairs);
/* the Newton solve of an Align's serial end (JacobiSVD(H).solve(b), ndt_omp_impl.hpp:127-129) as the device computes it, a lane
 * per system: H holds n row-major 6x6 matrices, b and x n 6-vectors.  Needs no cloud and no voxel table. */
smhip_status smhip_ndt_debug_solve6(smhip_handle h, int n, const double* H, const double* b, double* x);
/* parity-test hook: the fitness search of slots first_slot .. + npairs - 1 at the given poses (npairs column-major 4x4), through the
 * production path (the same launches as getFitnessScore).  d2 / stage: [npairs][capacity], row k = slot first_slot + k, entries in the
 * order the device holds the source (smhip_get_source_f32); entries past a slot's ns are left alone.  d2 = squared distance to the
 * nearest target point as the search found it (+inf for a query that is not finite); stage = the pass that settled the query:
 * 0 fine cube, 1 mid shells, 2 sweep over the voxel boxes, -1 where d2 is +inf.  scores[k] = the score the same pass reports.
 * SMHIP_ERR_NOT_READY before a slot's source and target are set; SMHIP_ERR_CAPACITY (nothing written) when capacity is below a
 * slot's source size. */
smhip_status smhip_ndt_debug_fitness(smhip_handle h, int first_slot, int npairs, const double* poses, int capacity,
                                     float* d2, int32_t* stage, double* scores);
/* measurement hook: `launches` back-to-back computeDerivatives launches (with Hessian) over slots first_slot .. + npairs - 1 at the
 * poses their last Align ended with, HIP events around them on the handle's stream: *ms_per_launch = the average duration of
 * the kernel, *pairs_per_launch = the (point, voxel) pairs one launch works through (for its algorithmic bytes).  The slots'
 * voxel tables must be current (an Align with the target cache on, or smhip_ndt_build_voxels for slot 0). */
smhip_status smhip_ndt_time_derivatives(smhip_handle h, int first_slot, int npairs, int launches, double* ms_per_launch,
                                        double* pairs_per_launch);

/* ---- registrators::NdtWithGicp (ndt_gicp.cc:28-112) ------------------------------------------
 * ApproximateVoxelGrid (0.2 m) on both clouds -> stock pcl NDT -> stock pcl GICP; PCL is not vendored by the
 * reference, the arithmetic follows PCL 1.8.1 (see oracle/ndt_gicp.py for the pinning).  The matcher keeps its
 * raw clouds in private device buffers and uses two pair slots of the handle per job as working space (job j: slot j and
 * slot pair_slots / 2 + j; the single Align is job 0), so the handle must be created with pair_slots >= 2,
 * max_source_points / max_target_points >= the raw cloud sizes and max_target_points >= the down-sampled source size.
 * One grid cell (gicp_search_cell) serves every search of an Align, so a target's search grid is built once per Align. */
typedef struct smhip_ndt_gicp_options {
  float voxel_resolution;              /* 0.2  ndt_gicp.h:73 */
  int32_t using_voxel_filter;          /* 1    ndt_gicp.h:74 */
  int32_t use_ndt;                     /* 1    ndt_gicp.h:75 */
  float ndt_transformation_epsilon;    /* 0.01 ndt_gicp.cc:38 */
  float ndt_step_size;                 /* 0.1  :39 */
  float ndt_resolution;                /* 1.0  :40 */
  int32_t ndt_max_iterations;          /* 35   :41 */
  int32_t gicp_max_iterations;         /* 35   :44 */
  double gicp_rotation_epsilon;        /* 1e-3 :43 */
  double gicp_transformation_epsilon;  /* 5e-4 PCL default (pclomp/gicp_omp.h:117) */
  double gicp_epsilon;                 /* 1e-3 (gicp_omp.h:109) */
  double gicp_corr_dist_threshold;     /* 5 m  (gicp_omp.h:118) */
  int32_t gicp_max_inner_iterations;   /* 20   (gicp_omp.h:112) */
  int32_t gicp_k_correspondences;      /* 20   (gicp_omp.h:108) */
  float gicp_search_cell;              /* grid cell (m) of the k-NN search behind the covariances; 0 = 3 x voxel_resolution.
                                          Performance only: the search is exact for any cell. */
  int32_t reserved[3];
} smhip_ndt_gicp_options;

typedef struct smhip_ndt_gicp_stats {
  int32_t ok;                          /* Align's bool: 0 when the NDT fitness was > 1 (result = guess) */
  int32_t n_source, n_target;          /* cloud sizes after the voxel filter */
  int32_t ndt_iterations;
  int32_t gicp_iterations;             /* outer iterations (nr_iterations_) */
  int32_t gicp_function_evaluations;   /* functor evaluations of all BFGS runs */
  int32_t gicp_correspondences;        /* kept correspondences of the last outer iteration */
  int32_t gicp_covariances_on_demand;  /* target covariances this Align estimated in its correspondence steps, each matched
                                          target point once (batches of >= 4 jobs; 0 where all were estimated up front) */
  double ndt_score;                    /* ndt_.getFitnessScore() (0.9 when use_ndt = 0) */
  double gicp_score;                   /* gicp_.getFitnessScore() (10 when skipped) */
} smhip_ndt_gicp_stats;

void smhip_ndt_gicp_default_options(smhip_ndt_gicp_options* o);
smhip_status smhip_ndt_gicp_set_options(smhip_handle h, const smhip_ndt_gicp_options* o);
/* SetInputSource / SetInputTarget of this matcher: raw clouds (stride 3, 4 or 5 floats), kept as handed over */
smhip_status smhip_ndt_gicp_set_source_f32(smhip_handle h, const float* xyz, int stride_floats, int n);
smhip_status smhip_ndt_gicp_set_target_f32(smhip_handle h, const float* xyz, int stride_floats, int n);
/* NdtWithGicp::Align.  *score = exp(-GICP fitness) (exp(-10) when stats->ok == 0, ndt_gicp.cc:103,107). */
smhip_status smhip_ndt_gicp_align(smhip_handle h, const double guess[16], double result[16], double* score,
                                  smhip_ndt_gicp_stats* stats);
/* Several NdtWithGicp pairs on one handle: a handle created with S pair slots runs S / 2 JOBS (smhip_ndt_gicp_jobs); job j has
 * its own clouds (the calls above are job 0's) and keeps its own target-derived structures between Aligns.
 * smhip_ndt_gicp_align_batch aligns jobs first_job .. first_job + njobs - 1 in lock-step -- the stages of
 * NdtWithGicp::Align (ndt_gicp.cc:55-112) run over all jobs at once, and inside NDT and GICP every job keeps the reference's own
 * sequence of evaluations while each round of evaluations is ONE launch and one hand-back for all jobs that are still
 * running (the back end's six concurrent SubmapPairMatch tasks, map_builder.cc:399-446, 655, as one call).  Results are
 * bit-identical to the single calls'.  guesses / results: njobs column-major 4x4; scores / stats: njobs entries (nullable). */
int smhip_ndt_gicp_jobs(smhip_handle h);
smhip_status smhip_ndt_gicp_set_source_f32_job(smhip_handle h, int job, const float* xyz, int stride_floats, int n);
smhip_status smhip_ndt_gicp_set_target_f32_job(smhip_handle h, int job, const float* xyz, int stride_floats, int n);
smhip_status smhip_ndt_gicp_align_batch(smhip_handle h, int first_job, int njobs, const double* guesses, double* results,
                                        double* scores, smhip_ndt_gicp_stats* stats);
/* pcl GICP alone on slot 0's clouds (smhip_set_source_f32 / smhip_set_target_f32); *fitness = getFitnessScore() */
smhip_status smhip_gicp_align(smhip_handle h, const double guess[16], double result[16], double* fitness,
                              smhip_ndt_gicp_stats* stats);
/* parity-test hooks: the working clouds of the last smhip_ndt_gicp_align in the filter's output order (which = 0
 * source, 1 target; xyz may be NULL to query the size) and the GICP covariances (n x 6 doubles: xx xy xz yy yz zz)
 * in that same order (or the upload order for smhip_gicp_align) */
smhip_status smhip_ndt_gicp_get_downsampled(smhip_handle h, int which, float* xyz, int capacity, int* n_out);
/* the GICP functor (value and 6-gradient, state x = tx ty tz roll pitch yaw) over the correspondences of the last outer
 * iteration of the last GICP run, with base_transformation_ = guess.  SMHIP_ERR_NO_MATCH when that step kept no
 * correspondence (the sums are divided by the kept count) */
smhip_status smhip_gicp_evaluate(smhip_handle h, const double guess[16], const double x[6], double* f, double grad[6]);
smhip_status smhip_gicp_get_covariances(smhip_handle h, int which, double* cov, int n);

/* ---- pre_processers::filter (pre_processors/filter_*.cc): the front end's pre-filters -----------
 * Range / AxisRange / BoundingBoxRemoval / RandomSampler / VoxelGrid applied in order to one cloud on the device,
 * as filter::Factory::Filter does (filter_factory.cc:83-106).  p[] carries each filter's float parameters:
 *   RANGE                 p[0] min_range, p[1] max_range
 *   AXIS_RANGE            p[0] min, p[1] max, axis_index 0 / 1 / 2
 *   RANDOM_SAMPLER        p[0] sampling_rate; seed selects the (counter-based) random stream
 *   VOXEL_GRID            p[0] voxel_size
 *   BOUNDING_BOX_REMOVAL  p[0..2] min_x min_y min_z, p[3..5] max_x max_y max_z */
enum { SMHIP_FILTER_RANGE = 1, SMHIP_FILTER_AXIS_RANGE = 2, SMHIP_FILTER_RANDOM_SAMPLER = 3, SMHIP_FILTER_VOXEL_GRID = 4,
       SMHIP_FILTER_BOUNDING_BOX_REMOVAL = 5 };
typedef struct smhip_filter_desc {
  int32_t type;
  int32_t axis_index;
  uint32_t seed;
  int32_t reserved;
  float p[6];
} smhip_filter_desc;
/* the filter's constructor defaults / its ConfigsValid() (1 = valid) */
void smhip_filter_default(int type, smhip_filter_desc* f);
int smhip_filter_config_valid(const smhip_filter_desc* f);
/* points: n rows of stride 4 (x y z intensity: KITTI; factor = i / n as the collector sets it,
 * builder/data/data_collector.h:202-204) or 5 floats (InnerPointType).  *n_out = size of the filtered cloud. */
smhip_status smhip_filter_chain_f32(smhip_handle h, const float* points, int stride_floats, int n,
                                    const smhip_filter_desc* chain, int n_filters, int* n_out);
/* the filtered cloud as InnerPointType rows (n x 5 floats) and, per point, the row of the input it came from
 * (inliers composed over the chain; -1 after a VoxelGrid).  Either pointer may be NULL. */
smhip_status smhip_filter_get_output(smhip_handle h, float* points5, int32_t* source_index, int n);
/* the filtered cloud becomes SetInputSource of `slot` without leaving the device */
smhip_status smhip_filter_output_to_source(smhip_handle h, int slot);
/* MotionCompensation (builder/map_builder.cc:232-257) of the filter workspace's current cloud by `delta` (column-major 4x4)
 * -> source of `slot`, on the device.  The workspace is left as it was, so the call can be repeated with another delta (the
 * front end compensates with the guess before Align and with the result after it).  points5_out (may be NULL): the compensated
 * cloud as InnerPointType rows in the workspace's row order.
 * Row i moves by common::InterpolateTransform(I, delta, factor_i) (common/math.h:199-211): Eigen's slerp from the identity to
 * delta's rotation (not normalised) and delta's translation times the factor, the product in double, each coordinate cast to
 * float; intensity and factor are carried.  The raw cloud gets into the workspace as for smhip_filter_output_to_source: a filter
 * chain (n_filters = 0 for an unfiltered scan; stride 4 rows get factor = i / n, stride 5 rows carry their own) or a built submap.
 * Refused before anything is touched: a bad slot, a null or non-finite delta, an empty cloud -- SMHIP_ERR_INVALID_ARGUMENT; no
 * cloud in the workspace -- SMHIP_ERR_NOT_READY; more rows than max_source_points -- SMHIP_ERR_CAPACITY.
 * A factor outside [0, 1] or NaN (the reference CHECK-aborts, math.h:202) is found by the kernel and reported through a flag:
 * SMHIP_ERR_INVALID_ARGUMENT AFTER the slot's source array was written.  The slot then has NO source (smhip_get_cloud_sizes
 * gives 0 and Align answers SMHIP_ERR_NOT_READY until a source is set again), points5_out is not written, and the workspace
 * still holds the cloud. */
smhip_status smhip_filter_output_to_source_compensated(smhip_handle h, int slot, const double delta[16], float* points5_out);

/* ---- the extended descriptor: every filter above plus GroundRemoval / GroundRemoval2 / RangeImage / StatisticRemoval ------
 * (pre_processors/filter_ground_removal.cc, filter_ground_removal2.cc, filter_range_image.cc Filter(); filter_statistic_removal.cc
 * gives StatisticRemoval's parameters only, what it computes is defined in DESIGN.md §6).  Slots:
 *   RANGE .. BOUNDING_BOX_REMOVAL  p[0..5] as in smhip_filter_desc, i[0] axis_index; seed as there
 *   GROUND_REMOVAL   p[0] leaf_size, p[1] height_threshold; i[0] min_point_num_in_voxel
 *   GROUND_REMOVAL2  p[0] r_max, p[1] r_min, p[2] start_ground_height, p[3] long_line_threshold, p[4] max_long_line_height,
 *                    p[5] max_start_height, p[6] max_error, p[7] max_slope, p[8] max_b (unused by the reference),
 *                    p[9] max_dist_to_line, p[10] search_angle; i[0] bin_num, i[1] segment_num, i[2] thread_num (ignored)
 *   RANGE_IMAGE      p[0] top_angle, p[1] btm_angle, p[2] offset_x, p[3] offset_y, p[4] offset_z;
 *                    i[0] vertical_line_num, i[1] horizontal_line_num
 *   STATISTIC_REMOVAL  p[0] std_mul; i[0] point_num_meank
 * Device limits (refused with SMHIP_ERR_INVALID_ARGUMENT): bin_num <= 4096, bin_num * segment_num <= 2^22, the search
 * of neighbouring segments within one turn, vertical_line_num * horizontal_line_num <= 2^22, voxel indices within +-2^20.
 * 1 <= point_num_meank <= 64 (a query's best-k set lives in LDS); std_mul must be finite.
 * Rows with a non-finite x, y or z are kept by both ground filters and by StatisticRemoval and dropped by RangeImage.
 * StatisticRemoval has NO coordinate range: it searches the cloud sorted along one axis, not a grid, so any finite coordinates are
 * answered exactly.  When no more than point_num_meank rows are finite it keeps every row, returns SMHIP_OK and leaves a
 * "warning: ..." in smhip_last_error.  smhip_filter_chain_f32 does not take the extended ids 6-9. */
enum { SMHIP_FILTER_GROUND_REMOVAL = 6, SMHIP_FILTER_GROUND_REMOVAL2 = 7, SMHIP_FILTER_RANGE_IMAGE = 8, SMHIP_FILTER_STATISTIC_REMOVAL = 9 };
typedef struct smhip_filter_desc_ex {
  int32_t type;
  uint32_t seed;
  int32_t i[4];
  float p[12];
} smhip_filter_desc_ex;
void smhip_filter_default_ex(int type, smhip_filter_desc_ex* f);
/* 1 = the reference accepts it and the device can hold it */
int smhip_filter_config_valid_ex(const smhip_filter_desc_ex* f);
/* smhip_filter_chain_f32 for extended descriptors; smhip_filter_get_output / _output_to_source read its result */
smhip_status smhip_filter_chain_ex_f32(smhip_handle h, const float* points, int stride_floats, int n,
                                       const smhip_filter_desc_ex* chain, int n_filters, int* n_out);
/* parity-test hook: what the last StatisticRemoval of the last filter chain computed.  distance (n floats, or NULL): the mean
 * distance to the point_num_meank nearest neighbours per row, in the row order that filter saw (n = its input size; 0 for a
 * non-finite row); stats (or NULL): sum and sum of squares of the finite rows' distances, their number V, and the threshold
 * mean + std_mul * stddev.  SMHIP_ERR_NOT_READY when no such filter ran in the last chain or it kept every row for V <= k. */
smhip_status smhip_filter_statistic_last(smhip_handle h, float* distance, int n, double stats[4]);

/* ---- Submap::InsertFrame for a full submap (builder/submap.cc:98-158) ---------------------------
 * Frame k = n[k] rows of `stride_floats` floats at rows[k] (4: x y z intensity, factor = i / n[k] of its own frame as the
 * collector sets it; 5: InnerPointType) and the column-major 4x4 local_poses + 16 k.  One kernel launch moves every frame into
 * the first frame's coordinates with the reference's TransformPoint (cloud_types.cc:167-178: the pose cast to float, x' = ((m00 x
 * + m01 y) + m02 z) + m03, every product and sum rounded to float), carries intensity and factor unchanged, concatenates the
 * frames in order and writes each row's VoxelGrid key; with voxel_size > 0 the VoxelGrid of the filters above follows (double
 * sums per voxel in frame order, then point order; output in the packed key's order), with voxel_size == 0
 * (enable_voxel_filter = false) the result is the plain concatenation.  The result becomes the filter workspace's current
 * cloud, on the device: smhip_filter_get_output and smhip_filter_output_to_source read it as they read a filter chain's
 * (source_index = the row in the concatenated input, -1 after the voxel filter), smhip_filter_output_to_target makes it a target.
 * Refused before anything is touched (the resident cloud stays as it was): n_frames < 1, a null table, a null frame of n[k] > 0, a
 * negative n[k], a stride other than 4 or 5, a non-finite pose, a voxel_size that is negative, not finite or in (0, 1e-6]
 * (VoxelGrid::ConfigsValid), every frame empty -- SMHIP_ERR_INVALID_ARGUMENT; more rows together than max(max_source_points,
 * max_target_points) -- SMHIP_ERR_CAPACITY.  Single empty frames among others are allowed.
 * Voxel indices beyond +-2^20 and non-finite rows are treated as smhip_filter_chain_f32's VoxelGrid treats them (the same key
 * function): a transformed row with an index beyond +-2^20, which includes an infinite coordinate, makes the call return
 * SMHIP_ERR_INVALID_ARGUMENT AFTER the rows were written, and the unfiltered concatenation is then the resident cloud, as the
 * chain leaves its input there; a NaN coordinate is not detected and enters the average of whatever voxel the rounding of NaN
 * selects.  With voxel_size == 0 no index is formed and every row is carried. */
smhip_status smhip_submap_build_f32(smhip_handle h, int n_frames, const float* const* rows, int stride_floats, const int* n,
                                    const double* local_poses, float voxel_size, int* n_out);
/* smhip_submap_build_f32 with every frame DE-SKEWED first ("Motion compensation after optimisation"):
 * motions holds 16 doubles per frame (column-major), the sensor's motion during that frame's sweep; a row goes through
 * MotionCompensation under its frame's motion (as smhip_filter_output_to_source_compensated computes it, the coordinates rounded to
 * float), then through the local TransformPoint.  Key, factor and source_index are smhip_submap_build_f32's.  The contract is that
 * call's, and a null or non-finite motion is refused before anything is touched.  A row whose factor is outside [0, 1] or NaN is
 * reported as the voxel index beyond +-2^20 is: SMHIP_ERR_INVALID_ARGUMENT after the rows were written (such a row is transformed as
 * it is), with the unfiltered concatenation as the resident cloud. */
smhip_status smhip_submap_build_compensated_f32(smhip_handle h, int n_frames, const float* const* rows, int stride_floats, const int* n,
                                                const double* local_poses, const double* motions, float voxel_size, int* n_out);
/* device CalculateNormals of the filter workspace's current cloud (a filter chain's output or a built submap) -> target of
 * `slot`, without a download (submap.cc:160-161); *n_out = the target's size.  SMHIP_ERR_NOT_READY when no cloud is there;
 * otherwise as smhip_prepare_target_f32 on the same rows. */
smhip_status smhip_filter_output_to_target(smhip_handle h, int slot, int* n_out);

/* ---- descriptor::M2dp (descriptor/m2dp.{h,cc}) -------------------------------------------------
 * The submap descriptor behind the loop detector's candidate search (builder/frame_base.cc:107-112,
 * back_end/loop_detector.cc:130-150), computed on the device in one submission: f64 moments of the rows, the PCA axes,
 * preProcess (m2dp.cc:45-70), the p*q signature histograms of singleViewProcess (:72-120) by integer atomics, and the first
 * singular pair of A (:140-147).  The descriptor is p*q + l*t floats, l = ceil(sqrt(max_distance / r)): the first left singular
 * vector followed by the first right one.  Two things the reference leaves open are defined in DESIGN.md section 6 ("M2DP"):
 * the PCA projection (mean and covariance / (N - 1) in double, eigenvalues descending, each of the first two axes signed so that
 * its largest-magnitude component is positive, third = first x second) and the sign of the singular pair (sum(u1) >= 0).
 * Same input, same bits: the moments are reduced in a fixed order and the histogram is integer.
 * Device limits: p * q <= 64 views and l * t <= 8192 columns. */
typedef struct smhip_m2dp_options {
  double r;                      /* 0.1 */
  double max_distance;           /* 100 */
  int32_t t, p, q;               /* 16, 4, 16 */
} smhip_m2dp_options;
void smhip_m2dp_default_options(smhip_m2dp_options* o);                                  /* M2dp::M2dp, m2dp.h:48-49 */
/* p*q + l*t, or -1 when the options are refused: null, r or max_distance not finite, r < 1e-6 (m2dp.cc:64), max_distance <= 0,
 * t, p or q < 1, or beyond the device limits above */
int smhip_m2dp_length(const smhip_m2dp_options* opts);
/* setInputCloud + getFinalDescriptor for n uploaded rows of `stride_floats` floats (4: x y z intensity, 5: InnerPointType); len
 * must equal smhip_m2dp_length(opts).  Nothing is allocated after a handle's first descriptor.
 * Refused before anything is touched: a null pointer, a stride other than 4 or 5, refused options, n < 2, a wrong len --
 * SMHIP_ERR_INVALID_ARGUMENT; n above max(max_source_points, max_target_points) -- SMHIP_ERR_CAPACITY.
 * Found by the kernels, SMHIP_ERR_INVALID_ARGUMENT afterwards with `descriptor` not written: a row with a non-finite coordinate;
 * no row within max_distance of the centroid (sigma1 = 0). */
smhip_status smhip_m2dp_f32(smhip_handle h, const float* points, int stride_floats, int n, const smhip_m2dp_options* opts,
                            float* descriptor, int len);
/* the same for the filter workspace's current cloud (a filter chain's output or a built submap): no download, and the workspace
 * is left as it was.  SMHIP_ERR_NOT_READY when no cloud is there. */
smhip_status smhip_m2dp_from_filter_output(smhip_handle h, const smhip_m2dp_options* opts, float* descriptor, int len);
/* parity-test hook: what the last descriptor call on the handle computed, for its n rows.  Any pointer may be NULL.  projected3:
 * 3 n floats, the rows after the PCA projection; kept: n words, 1 = getLength <= max_distance; A: the a_len = p*q*l*t counters,
 * row p*q_ + q, column l_index * t + t_index; n_kept: the kept rows.  SMHIP_ERR_NOT_READY when no call got as far as the
 * histogram. */
smhip_status smhip_m2dp_last(smhip_handle h, float* projected3, int32_t* kept, int32_t* A, int a_len, int* n_kept);
/* matchTwoM2dpDescriptors, m2dp.cc:151-169, on the host in double: -1 for a null pointer or n < 10 */
double smhip_m2dp_match(const float* P, const float* Q, int n);

/* ---- pose graph (what back_end::IsamOptimizer asks of GTSAM, back_end/isam_optimizer.{h,cc}) ----------
 * One rigid pose per node (a submap), between-factors on edges (odometry between consecutive submaps, loop edges from the loop
 * detector), nodes flagged `fixed` held where they are.  Defined in DESIGN.md section 6 ("Pose graph") and restated in
 * tests/pose_graph_ref.py -- GTSAM is third-party code the reference only calls:
 *   E = Z^-1 X_i^-1 X_j,  e = [Log_SO3(R_E); t_E] (rotation first),  cost = sum over edges of |e / sigma|^2,
 *   retraction R <- R Exp(dw), t <- t + R dv,
 * minimised from the given poses by Gauss-Newton steps with damping on a rejected step; each step's linear system by conjugate
 * gradients preconditioned with the block-tridiagonal part of the matrix (block cyclic reduction).  All f64, and ONE kernel
 * launch per call: nothing is read back between iterations.  Two calls on the same input give the same bits.
 * Beside the between-factor, smhip_pose_graph_*_factors take two more kinds, which carry the reference's GPS / ENU factors
 * (isam_optimizer.cc:238-349): a PRIOR on one node, and a POINT between a frame node and an observed node.
 * smhip_pose_graph_*_robust give any factor a Huber threshold ("Robust factors" below): the reference's Robust(Huber(1), ...) of
 * isam_optimizer.cc:90-93 and of the multi-trajectory optimiser's between-factors (multi_trajectory_optimizer.cc:68-81).
 * smhip_pose_graph_*_calib take a fourth kind, HANDEYE ("Odometry calibration factor" below): the reference's odometry calibration
 * factor through ODOM_CALIB_KEY (:84-93, 153-162, 209-224, 361-367), the place its IsamOptimizer puts its Huber model.
 * smhip_pose_graph_*_info let a BETWEEN carry a full 6x6 square-root information ("Edge information" below): the matcher's own,
 * where the reference weighs every scan-match edge with the same constants (:80-83).
 * The multi-trajectory optimiser and its builder (joining a second drive to a finished map) are host composition over these entries:
 * include/smhip/multi_trajectory.h.
 * Not restated: IMU, ViewGraph's picture output, the tf_error calibration point of enable_extrinsic_calib (GPS_CALIB_KEY), the geodetic
 * conversion to ENU, the loop detector's commented-out GPS guess (loop_detector.cc:291-300). */
#define SMHIP_POSE_GRAPH_MAX_NODES 8192
#define SMHIP_POSE_GRAPH_MAX_EDGES 32768
/* One launch runs at most this many conjugate-gradient iterations in all, whatever max_iterations and the per-solve cap allow, and
 * then stops with MAX_ITERATIONS at the poses of its last accepted step.  The per-solve cap alone, 12 x (non-chain edges) + 64, is
 * about 295 000 at the limits, times 50 steps: at the measured 0.2-0.3 ms per iteration that would hold the
 * device for an hour.  With this bound the worst accepted graph takes about a minute; a 909-node drive with 60 loop edges needs
 * 3 600 iterations, 0.65 s. */
#define SMHIP_POSE_GRAPH_MAX_PCG_TOTAL 200000
enum {
  SMHIP_POSE_GRAPH_STOP_STEP = 1,            /* max |delta| < 1e-10 */
  SMHIP_POSE_GRAPH_STOP_COST = 2,            /* a step lowered the cost by no more than 1e-12 of it */
  SMHIP_POSE_GRAPH_STOP_MAX_ITERATIONS = 3,  /* max_iterations steps, or SMHIP_POSE_GRAPH_MAX_PCG_TOTAL iterations inside them */
  SMHIP_POSE_GRAPH_STOP_DAMPING = 4,         /* every step up to lambda = 1e8 raised the cost */
  SMHIP_POSE_GRAPH_STOP_NUMERIC = 5          /* a pivot of the preconditioner's factorisation was not positive, or a sum not finite */
};
typedef struct smhip_pose_graph_options {
  int32_t max_iterations;       /* default 50: accepted and rejected steps together */
  int32_t reserved[3];
} smhip_pose_graph_options;
typedef struct smhip_pose_graph_stats {
  double initial_cost, final_cost;
  double damping;               /* lambda after the last step (lowered after an accepted one, also the one that stops) */
  int32_t stop_reason;          /* SMHIP_POSE_GRAPH_STOP_* */
  int32_t iterations;           /* steps tried = accepted_steps + rejected_steps, <= max_iterations */
  int32_t accepted_steps, rejected_steps;
  int32_t pcg_iterations;       /* summed over the steps */
  int32_t pcg_max_iterations;   /* the longest single solve, <= pcg_cap */
  int32_t pcg_cap;              /* 12 x (edges with |i - j| != 1) + 64 */
  int32_t levels;               /* of the cyclic reduction: the smallest L with 2^L >= n_nodes */
} smhip_pose_graph_stats;
void smhip_pose_graph_default_options(smhip_pose_graph_options* o);
/* The host half of smhip_pose_graph_optimize, which needs no device and no handle: its refusals, and on SMHIP_OK the list node ->
 * incident edges the kernel gathers in (csr_offsets: n_nodes + 1 words; csr_edges: 2 n_edges edge indices, ascending within a
 * node; either may be NULL).  why: the reason of a refusal, at most why_len bytes with the terminator (may be NULL). */
smhip_status smhip_pose_graph_plan(int n_nodes, const double* poses, const uint8_t* fixed, int n_edges, const int32_t* edge_ij,
                                   const double* edge_Z, const double* edge_sigmas, int32_t* csr_offsets, int32_t* csr_edges, char* why,
                                   int why_len);
/* poses_inout: n_nodes column-major 4x4; fixed: n_nodes bytes, non-zero = held; edge_ij: n_edges pairs (i, j); edge_Z: n_edges
 * column-major 4x4, the measured X_i^-1 X_j; edge_sigmas: 6 per edge, rotation first, or NULL for 0.1 x 3, 0.15 x 3
 * (isam_optimizer.cc:80-83); opts: NULL = defaults; stats: may be NULL.  The poses of free nodes are replaced, those of fixed
 * nodes are not written.  Device memory for the limits above is allocated at a handle's first call, nothing afterwards.
 * Refused before anything is touched, the poses left as given --
 *   SMHIP_ERR_INVALID_ARGUMENT: a null pointer, n_nodes < 1, an index out of range, i == j, a sigma that is not finite and positive,
 *     a non-finite pose or Z, a rotation block further than 1e-6 from orthonormal (or a reflection), a free node without an edge,
 *     a connected component without a fixed node, max_iterations < 1;
 *   SMHIP_ERR_CAPACITY: more nodes or edges than the limits (decided from the sizes alone: nothing is read or launched).
 * Found by the kernel, SMHIP_ERR_NO_MATCH afterwards with the poses left as given: stop_reason NUMERIC. */
smhip_status smhip_pose_graph_optimize(smhip_handle h, int n_nodes, double* poses_inout, const uint8_t* fixed, int n_edges,
                                       const int32_t* edge_ij, const double* edge_Z, const double* edge_sigmas,
                                       const smhip_pose_graph_options* opts, smhip_pose_graph_stats* stats);
/* parity-test hook: the first linearisation of the last smhip_pose_graph_optimize on the handle (at the poses that call was given),
 * computed again by one launch.  n_nodes, n_edges: what the caller's arrays are sized for; they must equal that call's sizes
 * (SMHIP_ERR_INVALID_ARGUMENT otherwise, nothing written).  Any pointer may be NULL.  residuals: 6 per edge, whitened (e / sigma); A, B: 36 per edge,
 * row-major, whitened; gradient: 6 per node (J^T r; zero for a fixed node); minv_v: M^-1 v for the caller's v (6 per node; entries
 * of fixed nodes are ignored and come back as zero), M = the block-tridiagonal part of H = J^T J.  SMHIP_ERR_NOT_READY when no
 * call got as far as the launch. */
smhip_status smhip_pose_graph_last(smhip_handle h, int n_nodes, int n_edges, double* residuals, double* A, double* B, double* gradient, const double* v, double* minv_v);
/* Factor kinds.  Every factor has an index pair (i, j), 16 doubles of data, 6 sigmas, and 6 rows of whitened A (for node i), B (for
 * node j) and residual:
 *   BETWEEN  as above: data = Z, column-major 4x4.
 *   PRIOR    on node i (j must equal i): data = a rigid pose P, column-major 4x4.  e = [Log_SO3(R_P^T R_i); R_P^T (t_i - t_P)],
 *            de/dxi_i = [Jr^-1(e_w), 0; 0, R_P^T R_i] in A; B is zero.  It is the BETWEEN from a constant node at P measured as the
 *            identity.  The node's list holds it once.
 *   POINT    between a frame node i and an observed node j != i: data[0..2] = l, the lever arm in node j's frame; data[3..5] = z,
 *            the measured point in the frame node i maps into; the rest is not read.  Three rows: r = R_i (R_j l + t_j) + t_i - z,
 *            whitened by sigmas[0..2] (sigmas[3..5] are not read); with p = R_j l + t_j, A = R_i [-hat(p), I], B = R_i R_j [-hat(l), I];
 *            rows 3..5 of A, B and the residual are zero.  The reference's transformFrom(compose(GPS_COORD, pose), lever) measured
 *            as enu (isam_optimizer.cc:238-261), to first order in the residual. */
#define SMHIP_POSE_GRAPH_FACTOR_BETWEEN 0
#define SMHIP_POSE_GRAPH_FACTOR_PRIOR 1
#define SMHIP_POSE_GRAPH_FACTOR_POINT 2
#define SMHIP_POSE_GRAPH_FACTOR_HANDEYE 3   /* the *_calib entries only: "Odometry calibration factor" below */
/* smhip_pose_graph_plan for factors of any kind.  kinds: one byte per factor, NULL = all BETWEEN; sigmas: NULL = the defaults of a
 * BETWEEN, refused when any other kind is present.  csr_edges: room for 2 n_factors indices; a PRIOR is listed once, so
 * csr_offsets[n_nodes] of them are written.  The refusals of smhip_pose_graph_optimize, and SMHIP_ERR_INVALID_ARGUMENT for: a kind
 * outside 0..2; a PRIOR with j != i or a P that is no rigid transform; a POINT with i == j or a non-finite l or z; a sigma that is
 * read and is not finite and positive; a free node with no BETWEEN and no PRIOR (POINT factors alone leave its block at rank 3); a
 * component -- connected by BETWEEN and POINT factors -- with neither a fixed node nor a PRIOR.  The non-chain edges of pcg_cap are
 * the BETWEEN and POINT factors with |i - j| != 1. */
smhip_status smhip_pose_graph_plan_factors(int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds,
                                           const int32_t* ij, const double* data, const double* sigmas, int32_t* csr_offsets,
                                           int32_t* csr_edges, char* why, int why_len);
/* smhip_pose_graph_optimize for factors of any kind: the same loop, constants, stop rules and limits (factors count as edges).  A
 * graph that passes the plan but leaves the preconditioner singular -- a chain run held by one or two POINT factors alone -- ends
 * as stop_reason NUMERIC / SMHIP_ERR_NO_MATCH with the poses left as given.  smhip_pose_graph_last serves whichever of the two
 * optimise calls ran last, n_edges being that call's factor count. */
smhip_status smhip_pose_graph_optimize_factors(smhip_handle h, int n_nodes, double* poses_inout, const uint8_t* fixed, int n_factors,
                                               const uint8_t* kinds, const int32_t* ij, const double* data, const double* sigmas,
                                               const smhip_pose_graph_options* opts, smhip_pose_graph_stats* stats);
/* Robust factors ("Robust factors"; tests/pose_graph_robust_ref.py).  A factor f of any kind may have a Huber
 * threshold k_f >= 0.  With s_f^2 = sum (e / sigma)^2 over its rows, its cost term is s_f^2 when k_f == 0 or s_f^2 <= k_f^2 and
 * 2 k_f s_f - k_f^2 otherwise (twice the Huber loss), and its weight w_f is 1 or k_f / s_f.  Linearisation makes the whitened rows as
 * without thresholds and multiplies them by sqrt(w_f) where w_f < 1 (GTSAM's Robust::WhitenSystem): J^T r is the exact gradient of
 * half the cost, H = sum w J^T J.  Damping, acceptance, stop rules, preconditioner and limits are untouched.  huber: one threshold
 * per factor, NULL = none; with NULL, zeros or thresholds never exceeded every output has the bits of the *_factors call.
 * Refused beside the refusals of the *_factors forms, before anything is touched: a threshold that is negative or not finite,
 * SMHIP_ERR_INVALID_ARGUMENT.
 * Two limits of the method: thresholds on the chain edges make the loop converge slowly (k = 1 on every factor of a 64-node ring with
 * one wrong loop edge: 50 steps without a stop), which is why smhip::back_end::IsamOptimizer offers them on loop edges only; and an
 * edge that claims two places 80 m apart coincide folds the ring with or without them -- the detector's distance gate comes first. */
smhip_status smhip_pose_graph_plan_robust(int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds,
                                          const int32_t* ij, const double* data, const double* sigmas, const double* huber,
                                          int32_t* csr_offsets, int32_t* csr_edges, char* why, int why_len);
smhip_status smhip_pose_graph_optimize_robust(smhip_handle h, int n_nodes, double* poses_inout, const uint8_t* fixed, int n_factors,
                                              const uint8_t* kinds, const int32_t* ij, const double* data, const double* sigmas,
                                              const double* huber, const smhip_pose_graph_options* opts, smhip_pose_graph_stats* stats);
/* The report of the last optimise call on the handle, whichever of the three it was, by one launch (one thread takes one factor):
 * per factor s_f (norm), w_f (weight) and the cost term (cost) at the poses that call's loop ENDED at.  Any pointer may be NULL.
 * After a call without thresholds every weight is 1.  SMHIP_ERR_INVALID_ARGUMENT when n_factors is not that call's count,
 * SMHIP_ERR_NOT_READY when no call got as far as the launch. */
smhip_status smhip_pose_graph_last_robust(smhip_handle h, int n_factors, double* norm, double* weight, double* cost);
/* Odometry calibration factor ("Odometry calibration factor"; tests/pose_graph_calib_ref.py).
 *   HANDEYE  between a frame node i (pose X) and a calibration node j != i (pose T): data = Z, a rigid pose, column-major 4x4 -- the
 *            odometer's pose relative to its first reading.  h = T^-1 X T, E = Z^-1 h, e = [Log_SO3(R_E); t_E], whitened by six
 *            sigmas.  With B_h = [Jr^-1(e_w), 0; 0, R_E] and Ad(G) = [R_G, 0; hat(t_G) R_G, R_G]:  A = B_h Ad(T^-1),
 *            B = B_h (I - Ad(h^-1)).  The reference's compose(between(calib_tf, pose), calib_tf) measured as
 *            Pose3(GetRelatedOdom()) (isam_optimizer.cc:215-223), to first order in the residual.  The model assumes the frame
 *            node of the first reading is at the identity.
 * The *_calib entries take the argument lists of the *_robust ones and accept kinds 0..3; every other entry keeps refusing kind 3.
 * Without a HANDEYE in the call every output has the bits of the *_robust call.  B vanishes where h is the identity and is
 * rank-deficient for planar motion (the z of t_T and a rotation of T about the common axis are not seen), so beside the refusals of
 * the *_robust forms, before anything is touched, SMHIP_ERR_INVALID_ARGUMENT for: a kind outside 0..3; a HANDEYE with i == j, a Z that
 * is no rigid transform or a sigma that is not finite and positive; a free node that is the j of a HANDEYE and carries no PRIOR.  For
 * its node i a HANDEYE counts like a BETWEEN (Ad is invertible); it connects components, and with |i - j| != 1 it is a non-chain edge
 * of pcg_cap.  Huber thresholds act on it as on the other kinds, s_f^2 over six rows.  smhip_pose_graph_last and
 * smhip_pose_graph_last_robust serve these calls too. */
smhip_status smhip_pose_graph_plan_calib(int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds,
                                         const int32_t* ij, const double* data, const double* sigmas, const double* huber,
                                         int32_t* csr_offsets, int32_t* csr_edges, char* why, int why_len);
smhip_status smhip_pose_graph_optimize_calib(smhip_handle h, int n_nodes, double* poses_inout, const uint8_t* fixed, int n_factors,
                                             const uint8_t* kinds, const int32_t* ij, const double* data, const double* sigmas,
                                             const double* huber, const smhip_pose_graph_options* opts, smhip_pose_graph_stats* stats);
/* Edge information ("Edge information"; tests/pose_graph_info_ref.py).  A BETWEEN factor may carry a full 6x6
 * square-root information L (row-major; the factor's information is L^T L) in place of its six inverse sigmas: rw = L e, A_w = L A,
 * B_w = L B, s_f^2 = |L e|^2, with e, A and B the unwhitened residual and Jacobians above; Huber acts on s_f as before.  This is how
 * the matcher's own information (smhip_icp_information, include/smhip/edge_information.h) reaches the optimiser.
 * The *_info entries take the argument lists of the *_calib ones plus, after huber: info_index, one per factor -- -1 = use the sigmas,
 * otherwise the index of an entry of sqrt_info, below n_factors -- or NULL = none; sqrt_info, 36 doubles per entry.  With info_index
 * NULL or all -1 every output has the bits of the *_calib call.  A factor with an L still needs valid sigmas; the kernel does not
 * read them.  Refused beside the refusals of the *_calib forms, before anything is touched, SMHIP_ERR_INVALID_ARGUMENT: an index
 * below -1 or not below n_factors; an L on a factor that is no BETWEEN; an L with a non-finite entry; a singular L (the smallest pivot
 * of an LU with partial pivoting at or below 1e-12 times its largest entry).  smhip_pose_graph_last and smhip_pose_graph_last_robust
 * serve these calls too. */
smhip_status smhip_pose_graph_plan_info(int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds,
                                        const int32_t* ij, const double* data, const double* sigmas, const double* huber,
                                        const int32_t* info_index, const double* sqrt_info, int32_t* csr_offsets, int32_t* csr_edges,
                                        char* why, int why_len);
smhip_status smhip_pose_graph_optimize_info(smhip_handle h, int n_nodes, double* poses_inout, const uint8_t* fixed, int n_factors,
                                            const uint8_t* kinds, const int32_t* ij, const double* data, const double* sigmas,
                                            const double* huber, const int32_t* info_index, const double* sqrt_info,
                                            const smhip_pose_graph_options* opts, smhip_pose_graph_stats* stats);
/* Marginal covariances ("Marginal covariances"; tests/pose_graph_marginals_ref.py): how well each pose is known --
 * what the reference asks of gtsam::Marginals::marginalCovariance (back_end/isam_optimizer.h:32).
 *   H = sum_f w_f J_f^T J_f is the Gauss-Newton matrix of the LAST optimise call on the handle, whichever of the five entries it was:
 *   the rows whitened (Huber weights and square-root informations applied as the linearisation applies them), at the poses that call's
 *   loop ENDED at (the state smhip_pose_graph_last_robust reports on), lambda = 0, fixed nodes left out.
 *   For a free node k:  Sigma_k = (X + X^T) / 2 with X = [H^-1]_kk, a 6x6 in the optimiser's tangent chart, rotation first:
 *   R <- R Exp(dw), t <- t + R dv, so its translation part is in the node's BODY frame; the world-frame position covariance is
 *   R_k Sigma_vv R_k^T.  For a fixed node Sigma_k = 0.  Cross blocks [H^-1]_{r,k} (row node r, column node k) come from the same
 *   solves, unsymmetrised; a cross block with a fixed node is 0.
 * Covariances are relative to the gauge: the held nodes, or the PRIOR factors.  With node 0 held, Sigma_k says how well node k is
 * known relative to node 0, not in the world.
 * Column c of node k solves H x = e_{6k+c} by the optimiser's own conjugate gradients from x = 0, preconditioned by the
 * block-tridiagonal part of H, stopped at r^T M^-1 r <= (1e-10)^2 r0^T M^-1 r0 and capped at that call's pcg_cap.  Two launches: one
 * workgroup linearises and factors, then min(n_query, max_workgroups) workgroups take the queries w, w + G, w + 2G, ..., six solves
 * each.  A query's bits do not depend on the workgroup that ran it, on max_workgroups or on what else was queried.
 * query: n_query node indices (repeats allowed); cov: 36 doubles per query, row-major.  rows: n_rows node indices and blocks:
 * n_query x n_rows x 36 doubles, block (q, r) = [H^-1]_{rows[r], query[q]}, row-major; n_rows 0 with NULLs for none.  opts: NULL =
 * defaults; stats: may be NULL.  The poses, and what smhip_pose_graph_last and smhip_pose_graph_last_robust return afterwards, are
 * not changed.  The workspace, (7 x 6 n_nodes + 6 n_factors) doubles per workgroup, is grown to fit a call and never shrunk.
 * Refused before anything is touched, nothing written --
 *   SMHIP_ERR_NOT_READY: no optimise call reached its launch, or the last one ended NUMERIC;
 *   SMHIP_ERR_INVALID_ARGUMENT: n_nodes is not the last call's, n_query < 1, a null query or cov, an index out of range, n_rows > 0
 *     with a null rows or blocks, max_workgroups < 0;
 *   SMHIP_ERR_CAPACITY, from the sizes alone: ceil(n_query / G) x 6 x pcg_cap > SMHIP_POSE_GRAPH_MAX_PCG_TOTAL (ask in several calls).
 *     max_workgroups above 4 per CU is clamped to that (a workgroup of 1024 threads fills a CU, and each costs a slice of the workspace);
 *     cov and blocks together more than 2^27 doubles (1 GiB) are refused likewise.
 * Found by the kernels, SMHIP_ERR_NO_MATCH with cov and blocks not written: a pivot of the factorisation that is not positive; a
 * column whose solve ended without meeting the tolerance -- at pcg_cap, or because a sum was not positive or not finite (stats are
 * written in this case; pcg_iterations saturates at INT32_MAX).
 * Out of scope: using the covariances inside LoopDetector's distance gate (the obvious follow-up; the covariance can also size the
 * window of smhip_guess_search_f32 below, which is what makes a wider gate useful), a selected-inversion shortcut for
 * the chain part, joint marginals of more than two nodes, incremental reuse between calls. */
typedef struct smhip_pose_graph_marginals_options {
  int32_t max_workgroups;       /* 0 = one per CU */
  int32_t reserved[3];
} smhip_pose_graph_marginals_options;
typedef struct smhip_pose_graph_marginals_stats {
  int32_t workgroups;           /* G */
  int32_t pcg_iterations;       /* summed over every column of every query */
  int32_t pcg_max_iterations;   /* the longest single column, <= pcg_cap */
  int32_t pcg_cap;              /* the last optimise call's */
} smhip_pose_graph_marginals_stats;
void smhip_pose_graph_marginals_default_options(smhip_pose_graph_marginals_options* o);
smhip_status smhip_pose_graph_marginals(smhip_handle h, int n_nodes, int n_query, const int32_t* query, double* cov, int n_rows,
                                        const int32_t* rows, double* blocks, const smhip_pose_graph_marginals_options* opts,
                                        smhip_pose_graph_marginals_stats* stats);

/* ---- correlative guess search ("Guess search"; tests/guess_search_ref.py) ----------
 * Not in the reference: LoopDetector::CloseLoop (back_end/loop_detector.cc:282-318) starts its ICP from the drifted poses, and a local
 * ICP has no capture range of metres.  Given a target cloud, a source cloud and a guess, every transform of a window around the guess
 * is scored by how many source points land in an occupied target voxel, and the best one is returned.  All integers after rule 5:
 *  1 rows       rows with a non-finite x, y or z are dropped from both clouds (icp_pointmatcher.cc:57-66)
 *  2 sample     n source rows left, M = max_source_points: all of them if n <= M, else rows floor(k n / M), k = 0 .. M-1 (64-bit)
 *  3 target     v = floorf(p / resolution) per axis, the f32 IEEE quotient; occupancy is a bitmap over the box of the target's v
 *  4 yaws       a = -yaw_steps .. yaw_steps: R_a = Rz(a * yaw_step) * R0 about the TARGET frame's z, t0 kept; R0, t0 from the guess;
 *               formed in double on the host (c r0 - s r1 and s r0 + c r1 per column, each product and sum rounded), cast to f32
 *  5 source     q = ((r00 x + r01 y) + r02 z) + t per row of R_a, every f32 product and sum rounded on its own; w = floorf(q / res)
 *  6 score      score(a, i, j, k) = #{sampled source points : w + (i, j, k) is an occupied target voxel}, i, j in [-half_xy, half_xy],
 *               k in [-half_z, half_z]; a voxel outside the bitmap is empty.  Flat index ((a + yaw_steps) * nz + (k + half_z)) * nxy^2 +
 *               (j + half_xy) * nxy + (i + half_xy) with nxy = 2 half_xy + 1, nz = 2 half_z + 1
 *  7 pick       the highest score; among equals the smallest i^2 + j^2 + k^2, then the smallest |a|, then the smallest a, k, j, i --
 *               taken from the stored score volume under that total order, so it does not depend on scheduling
 *  8 result     rotation Rz(a* yaw_step) R0 and translation t0 + resolution * (i*, j*, k*), in double
 *  9 also       guess_score = score(0, 0, 0, 0); runner_up_score = the best score among candidates with max(|i-i*|, |j-j*|, |k-k*|) > 2
 *               or |a-a*| > 1, 0 if there is none: whether the peak stands alone
 * Refused from the sizes alone, before anything is touched, `result` not written --
 *   SMHIP_ERR_INVALID_ARGUMENT: a null pointer, a stride other than 4 (x y z intensity) or 5 (InnerPointType), a cloud of no row, a
 *     resolution that is not finite and positive, a negative half_xy, half_z or yaw_steps, a yaw_step that is not finite,
 *     max_source_points < 1, a guess with an entry that is not finite;
 *   SMHIP_ERR_CAPACITY: more than 2^25 candidates (the score volume is one int32 each), a half-width above 2^19, a cloud of more
 *     rows than max(max_source_points, max_target_points) of the handle.
 * Found later, `result` not written: a cloud with no finite row -- SMHIP_ERR_INVALID_ARGUMENT (seen while the rows are staged for
 *   upload; rules 1 and 2 are applied there); a voxel coordinate of either cloud at or beyond 2^30, a target box that with the window
 *   exceeds 2^20 voxels along an axis, a bitmap above 2^28 bits -- SMHIP_ERR_CAPACITY (the box comes from a device reduction).
 * The workspace (clouds, bitmap, (2 yaw_steps + 1) x n_source_used packed voxels, the score volume) grows to fit a call and never
 * shrinks: nothing is allocated by a call no larger than an earlier one.  Same input, same bits.
 * Out of scope: sizing the window from smhip_pose_graph_marginals, roll and pitch, resident clouds without upload, multi-GPU. */
typedef struct smhip_guess_search_options {
  float resolution;              /* 0.5 (metres per voxel) */
  int32_t max_source_points;     /* 4096 */
  int32_t half_xy, half_z;       /* 20, 2 (voxels) */
  int32_t yaw_steps;             /* 10 */
  int32_t reserved;
  double yaw_step;               /* 2 degrees, in radians */
} smhip_guess_search_options;
typedef struct smhip_guess_search_result {
  double transform[16];          /* column-major, rule 8 */
  int32_t best_score, guess_score, runner_up_score;
  int32_t n_source_used, n_candidates;
  int32_t best_yaw, best_i, best_j, best_k;     /* a*, i*, j*, k* */
  int32_t reserved[3];
} smhip_guess_search_result;
void smhip_guess_search_default_options(smhip_guess_search_options* o);
/* guess: 16 doubles, column-major */
smhip_status smhip_guess_search_f32(smhip_handle h, const float* target, int n_target, int target_stride, const float* source, int n_source,
                                    int source_stride, const double* guess, const smhip_guess_search_options* opts,
                                    smhip_guess_search_result* result);
/* parity-test hook: what the last completed search on the handle left.  Any pointer may be NULL.  volume: the volume_len =
 * n_candidates scores in the flat order of rule 6; origin3 / extent3: the bitmap's box in voxels; source_voxels: voxels_len = 3 x
 * (2 yaw_steps + 1) x n_source_used words, w of rule 5 per yaw and sampled point -- INT32_MIN three times for a point that no offset of
 * the window brings into the box (it is stored as such).  SMHIP_ERR_NOT_READY when no search has completed. */
smhip_status smhip_guess_search_last(smhip_handle h, int32_t* volume, int volume_len, int32_t* origin3, int32_t* extent3, int32_t* source_voxels,
                                     int voxels_len);

/* ---- static_map::MultiResolutionVoxelMap (builder/multi_resolution_voxel_map.{h,cc}) ----------
 * The probabilistic hit / miss voxel map with ray casting behind the reference's static-map output (one
 * InsertPointCloud per frame, builder/map_builder.cc:832-900), on the device.  Results equal the reference's insert loop
 * executed in point order (its OpenMP form races on the probabilities, multi_resolution_voxel_map.cc:76-94).
 * Field names and defaults: MrvmSettings, multi_resolution_voxel_map.h:54-65. */
typedef struct smhip_mrvm_settings {
  float prob_threshold;          /* 0.6 */
  float high_resolution;         /* 0.1 m voxels */
  float hit_prob;                /* 0.55, clamped to [0.501, 0.9] (.cc:50) */
  float miss_prob;               /* 0.48, clamped to [0.1, 0.499] (.cc:51) */
  float z_offset;                /* added to the origin's z (.cc:66-67) */
  int32_t max_point_num_in_cell; /* 10 */
  int32_t use_max_intensity;     /* 1: output points carry their voxel's max intensity (.cc:160-163) */
  int32_t reserved;
} smhip_mrvm_settings;
typedef struct smhip_mrvm_context* smhip_mrvm_handle;
void smhip_mrvm_default_settings(smhip_mrvm_settings* s);
/* table_log2: the open-addressing voxel table STARTS with 2^table_log2 slots and doubles between inserts, like the reference's
 * map grows: before an insert it is made large enough for the voxels it holds plus one per point of the coming cloud to fill at
 * most half of it, up to 2^28 slots (smhip_mrvm_set_max_table_log2 lowers that; a slot costs 37 + 20 * max_point_num_in_cell
 * bytes).  Only a table that can no longer grow (the limit, or the device's memory) reports "> 70 % full" as a warning and, when
 * a voxel finds no slot, SMHIP_ERR_CAPACITY from then on (the voxel is lost, the rest of the cloud is applied).
 * max_cloud_points: the largest cloud one InsertPointCloud may hand over */
smhip_status smhip_mrvm_create(int device, int table_log2, int max_cloud_points, const smhip_mrvm_settings* settings, smhip_mrvm_handle* out);
smhip_status smhip_mrvm_destroy(smhip_mrvm_handle h);
const char* smhip_mrvm_last_error(smhip_mrvm_handle h);
void smhip_mrvm_set_offset_z(smhip_mrvm_handle h, float offset);                         /* SetOffsetZ, .cc:55-57 */
/* InsertPointCloud(cloud, origin), .cc:59-131: n rows of `stride_floats` >= 4 floats (x y z intensity [factor]: InnerPointType is
 * stride 5), origin = the sensor position of the frame.  Non-finite points are skipped.  Refused BEFORE the map is touched
 * (status != OK, map unchanged): empty cloud, cloud larger than max_cloud_points, origin not finite or beyond +-2^20 voxels.
 * Applied with a warning (status OK, text in smhip_mrvm_last_error): points beyond +-2^20 voxels are skipped (their number:
 * smhip_mrvm_last_skipped; the flag does not carry over to the next insert), a table > 70 % full that cannot grow. */
smhip_status smhip_mrvm_insert_f32(smhip_mrvm_handle h, const float* points, int stride_floats, int n, const float origin[3]);
/* ApplyTransformToOutput(pose) + InsertPointCloud(cloud, pose translation), map_builder.cc:842-848: n raw rows of `stride_floats`
 * floats (4: KITTI x y z reflectance, factor = 0; 5: InnerPointType) go up as they are, and a kernel writes the world-frame rows
 * with the reference's TransformPoint (builder/data/cloud_types.cc:167-178): the matrix cast to float, x' = ((m00 x + m01 y) +
 * m02 z) + m03 with every product and sum rounded to float (no fused multiply-add, as the reference's -O2 build without -march);
 * intensity = row[3] * intensity_scale in float (255 for raw KITTI rows, kitti_reader.cc:113).  pose: column-major 4x4; origin =
 * its translation cast to float.  Refused before the map is touched: a non-finite pose, a stride other than 4 or 5, and
 * everything smhip_mrvm_insert_f32 refuses; warnings as there. */
smhip_status smhip_mrvm_insert_transformed_f32(smhip_mrvm_handle h, const float* rows, int stride_floats, int n, const double pose[16],
                                               float intensity_scale);
/* Motion compensation after optimisation: smhip_mrvm_insert_transformed_f32 of the frame DE-SKEWED by `motion`,
 * the sensor's motion during the frame's sweep (column-major 4x4; pose^-1 * the next frame's pose), `pose` being the sensor pose at
 * the START of the sweep.  One kernel per row: MotionCompensation (map_builder.cc:232-257) exactly as
 * smhip_filter_output_to_source_compensated computes it (InterpolateTransform(I, motion, factor) in double, each coordinate cast to
 * float), then TransformPoint under `pose` as above; the de-skewed cloud is never stored.  The factor is the row's fifth float
 * (stride 5) or the collector's (float)((double)i / n) (stride 4) and is carried into the stored point; the ray origin stays the
 * pose's translation cast to float.  Refused before the map is touched: a null or non-finite motion and everything
 * smhip_mrvm_insert_transformed_f32 refuses.  A row whose factor is outside [0, 1] or NaN: SMHIP_ERR_INVALID_ARGUMENT with the map
 * bit for bit as it was (the kernel's flag is read before any kernel that writes the table runs, which costs one stream
 * synchronise the plain insert does not have). */
smhip_status smhip_mrvm_insert_compensated_f32(smhip_mrvm_handle h, const float* rows, int stride_floats, int n, const double pose[16],
                                               const double motion[16], float intensity_scale);
smhip_status smhip_mrvm_last_skipped(smhip_mrvm_handle h, int* n);
smhip_status smhip_mrvm_voxel_count(smhip_mrvm_handle h, int* n);
smhip_status smhip_mrvm_set_max_table_log2(smhip_mrvm_handle h, int max_table_log2);   /* 10..28; default 28 */
int smhip_mrvm_table_log2(smhip_mrvm_handle h);                                        /* log2 of the table's current size */
/* OutputToPointCloud(threshold, PointXYZI cloud) without averaging, .cc:133-170: rows x y z intensity of every stored point of
 * every voxel with probability byte >= uint8(threshold * 256), in no particular order (the reference iterates an unordered
 * map).  capacity = 0 only counts. */
smhip_status smhip_mrvm_output(smhip_mrvm_handle h, float threshold, float* xyzi, int capacity, int* n_out);
/* Both OutputToPointCloud overloads with MrvmSettings::output_average, .cc:125-216.  flags: SMHIP_MRVM_AVERAGE = one row per
 * voxel, the float mean of its stored points (summed in their order, divided by float(size)); its 4th column is the voxel's max
 * intensity, or 0 without use_max_intensity (the reference never assigns it).  SMHIP_MRVM_RGB = the PointXYZRGB overload: the
 * 4th column holds the bits of the packed colour a << 24 | r << 16 | g << 8 | b with r = g = b = min(255, uint32(max_intensity * 1.4))
 * and a = 255 (pcl::PointXYZRGB's `rgb` float; the reference assigns r, g, b only, so the alpha byte is what the PCL >= 1.8
 * constructor puts there). */
#define SMHIP_MRVM_AVERAGE 1
#define SMHIP_MRVM_RGB 2
/* SMHIP_MRVM_SORTED (combinable with the two above): rows ordered by the packed voxel key ascending -- x, then y, then z of the
 * voxel, each as a signed integer -- and within a voxel in stored-point order; the order is computed on the device (a radix sort
 * of the voxels by key and an exclusive scan of their row counts), so the same map gives the same rows on every call and run.
 * Without it the rows come in table order, as before. */
#define SMHIP_MRVM_SORTED 4
smhip_status smhip_mrvm_output_ex(smhip_mrvm_handle h, float threshold, int flags, float* rows, int capacity, int* n_out);
/* parity-test hook: every voxel of the map -- key (3 ints), probability byte, max intensity, number of stored points and
 * the points themselves (max_point_num_in_cell x 5 floats per voxel), in no particular order */
smhip_status smhip_mrvm_dump(smhip_mrvm_handle h, int32_t* keys3, uint8_t* prob, int32_t* max_intensity, int32_t* npoints, float* points5,
                             int capacity, int* n_out);

/* ---- the map package (SaveTrajectoriesAsMapPackage, builder/map_package.{h,cc}) ----------
 * The static map cut into overlapping square pieces: three calls on a voxel map that a piece's map is built and cut with, and
 * the host-only plan of the pieces.  include/smhip/map_package.h drives them and writes the files. */
/* smhip_mrvm_insert_transformed_f32 of the rows whose TRANSFORMED x, y lie in the closed box [bb_min, bb_max] (map_package.cc:
 * 169-179): the float coordinates widened to double against the double bounds, so a NaN coordinate fails; the rows kept stay in
 * their order (a scan of the keep flags places them, no atomic) and the insert runs over exactly those.  The transform's
 * arithmetic is smhip_mrvm_insert_transformed_f32's; the origin is the pose's translation cast to float.  n_kept (may be NULL):
 * the rows kept.  None kept: SMHIP_OK, the map bit for bit as it was (the reference makes no insert then, :177-180).  Refused before
 * the map is touched: everything smhip_mrvm_insert_transformed_f32 refuses, and a bound that is not finite. */
smhip_status smhip_mrvm_insert_transformed_clipped_f32(smhip_mrvm_handle h, const float* rows, int stride_floats, int n, const double pose[16],
                                                       float intensity_scale, const double bb_min[2], const double bb_max[2], int* n_kept);
/* smhip_mrvm_output_ex's SORTED rows (flags: SMHIP_MRVM_AVERAGE and SMHIP_MRVM_RGB; SORTED is implied) of which only those inside
 * the closed box are written, recentred: x <- float(double(x) - centre[0]), the same for y (map_package.cc:191-197).  The test is on
 * the output row -- with AVERAGE on the averaged row, not on the stored points.  capacity = 0 only counts.  Refused: a bound or a
 * centre that is not finite. */
smhip_status smhip_mrvm_output_clipped(smhip_mrvm_handle h, float threshold, int flags, const double bb_min[2], const double bb_max[2],
                                       const double centre[2], float* rows, int capacity, int* n_out);
/* Empties the map by a kernel; the table keeps its current size (a handle reused for the next piece allocates nothing). */
smhip_status smhip_mrvm_clear(smhip_mrvm_handle h);
typedef struct smhip_map_package_options {
  double border_offset;          /* 100: widens the extent, and a piece's box when its submaps are chosen */
  double piece_width;            /* 500: pieces are piece_width wide and piece_width / 2 apart */
  int32_t reserved[4];
} smhip_map_package_options;
void smhip_map_package_default_options(smhip_map_package_options* o);
#define SMHIP_MAP_PACKAGE_MAX_PIECES 65536
/* The plan (map_package.cc:59-141), on the host: needs no device and no handle.  translations: n_submaps x 3 doubles (x y z of
 * every submap's global pose, in trajectory order).  steps: x_steps, y_steps; piece (x, y) is entry x * y_steps + y of centres
 * (2 doubles), boxes (min x, min y, max x, max y) and member_offsets (pieces + 1 words into members, the submaps a piece is
 * built from, ascending).  n_members: the length of members.  The arrays are filled when piece_capacity >= pieces (members when
 * member_capacity >= n_members as well); with smaller capacities the call only counts.  Any output pointer but steps may be NULL.
 * SMHIP_ERR_INVALID_ARGUMENT, the reason in why (at most why_len bytes with the terminator; may be NULL): a negative step count
 * (the reference's refusal), and, not the reference's: no submap, a translation or border_offset that is not finite, a piece_width
 * that is not finite and positive, more than SMHIP_MAP_PACKAGE_MAX_PIECES pieces. */
smhip_status smhip_map_package_plan(int n_submaps, const double* translations, const smhip_map_package_options* opts, int32_t steps[2],
                                    int piece_capacity, double* centres, double* boxes, int32_t* member_offsets, int member_capacity,
                                    int32_t* members, int32_t* n_members, char* why, int why_len);

/* ---- profiling ----------------------------------------------------------- */
/* enable: 0 off, 1 events around every launch; events around ONE kernel class only, cheap enough to leave on inside a timed
 * region: 2 the NN kernels proper (fused search / full walk, certificate pass), 3 accumulate, 4 the listed search */
smhip_status smhip_icp_enable_profile(smhip_handle h, int enable);
smhip_status smhip_icp_get_profile(smhip_handle h, smhip_icp_profile* out);
/* queries that went through a search (exact modes: certificate failed; NABO: walked again) in iterations 0..11 of the
 * slot's last Align; counts[12] */
smhip_status smhip_icp_get_search_counts(smhip_handle h, int slot, uint32_t* counts);

#ifdef __cplusplus
}
#endif
#endif /* SMHIP_H_ */
