// pose_graph_plan.h -- what smhip_pose_graph_optimize decides on the host before anything reaches the device: the refusals of
// include/smhip.h ("pose graph") and the node -> incident-edges list the kernel gathers in.  Plain C++, no HIP: the library's
// smhip_pose_graph_plan hands it out, and tests/cpp/test_pose_graph.cc includes it directly.
#pragma once
#include <cmath>
#include <cstdint>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/smhip.h"

namespace smhip {
namespace pose_graph {

constexpr int kMaxNodes = SMHIP_POSE_GRAPH_MAX_NODES, kMaxEdges = SMHIP_POSE_GRAPH_MAX_EDGES;
constexpr double kDefaultSigmas[6] = {0.1, 0.1, 0.1, 0.15, 0.15, 0.15};      // isam_optimizer.cc:80-83
constexpr double kOrthonormalTolerance = 1.0e-6;

struct Plan {
  std::vector<int32_t> csr_offsets;      // n_nodes + 1
  std::vector<int32_t> csr_edges;        // 2 n_edges less the PRIORs: the factors of node k, ascending, at [csr_offsets[k], csr_offsets[k + 1])
  int non_chain_edges = 0;               // BETWEEN, POINT and HANDEYE factors with |i - j| != 1
  int pcg_cap = 0;                       // 12 non_chain_edges + 64
  int levels = 0;                        // of the cyclic reduction: the smallest L with 2^L >= n_nodes
};

// nullptr, or what is wrong with a column-major 4x4 rigid transform
inline const char* transform_problem(const double* m) {
  for (int k = 0; k < 16; ++k) if (!std::isfinite(m[k])) return "is not finite";
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) {
      double s = 0.0;
      for (int r = 0; r < 3; ++r) s += m[4 * a + r] * m[4 * b + r];          // columns a and b
      if (std::fabs(s - (a == b ? 1.0 : 0.0)) > kOrthonormalTolerance) return "has a rotation block further than 1e-6 from orthonormal";
    }
  const double det = m[0] * (m[5] * m[10] - m[6] * m[9]) - m[4] * (m[1] * m[10] - m[2] * m[9]) + m[8] * (m[1] * m[6] - m[2] * m[5]);
  if (!(det > 0.0)) return "has a reflection for its rotation block";
  return nullptr;
}

// SMHIP_OK and the plan, or the refusal with its reason in *why.  Reads nothing beyond the sizes it has accepted.  kinds: one
// SMHIP_POSE_GRAPH_FACTOR_* per factor, nullptr = every factor a BETWEEN.  data: 16 doubles per factor -- BETWEEN the measurement and
// PRIOR the pose, column-major 4x4; POINT the lever arm (0..2) and the measured point (3..5).
// calib: HANDEYE factors (data: the odometer's pose, column-major 4x4) are accepted too -- the *_calib entries; without it kind 3 is
// refused in the words it always was.
inline smhip_status check_and_plan_kinds(bool calib, int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds, const int32_t* ij,
                                         const double* data, const double* sigmas, Plan* plan, std::string* why) {
  auto refuse = [&](smhip_status s, const std::string& text) { if (why) *why = "pose graph: " + text; return s; };
  if (!poses || !fixed || (n_factors > 0 && (!ij || !data))) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "null pointer");
  if (n_nodes < 1 || n_factors < 0) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "at least one node and no negative edge count");
  if (n_nodes > kMaxNodes) return refuse(SMHIP_ERR_CAPACITY, "more than " + std::to_string(kMaxNodes) + " nodes");
  if (n_factors > kMaxEdges) return refuse(SMHIP_ERR_CAPACITY, "more than " + std::to_string(kMaxEdges) + " edges");
  for (int k = 0; k < n_nodes; ++k)
    if (const char* p = transform_problem(poses + 16 * (size_t)k)) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "pose " + std::to_string(k) + " " + p);
  std::vector<int32_t> parent((size_t)n_nodes), degree((size_t)n_nodes, 0);
  std::vector<uint8_t> held((size_t)n_nodes, 0), prior((size_t)n_nodes, 0);      // by a BETWEEN or a PRIOR: all six directions; by a PRIOR
  std::vector<uint8_t> calibrated((size_t)n_nodes, 0);                           // the j of a HANDEYE
  std::iota(parent.begin(), parent.end(), 0);
  auto root = [&](int a) { while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; } return a; };
  int non_chain = 0;
  for (int e = 0; e < n_factors; ++e) {
    const int i = ij[2 * e], j = ij[2 * e + 1];
    const int kind = kinds ? kinds[e] : SMHIP_POSE_GRAPH_FACTOR_BETWEEN;
    const double* dat = data + 16 * (size_t)e;
    const std::string name = "edge " + std::to_string(e);
    const bool handeye = calib && kind == SMHIP_POSE_GRAPH_FACTOR_HANDEYE;
    if (kind != SMHIP_POSE_GRAPH_FACTOR_BETWEEN && kind != SMHIP_POSE_GRAPH_FACTOR_PRIOR && kind != SMHIP_POSE_GRAPH_FACTOR_POINT && !handeye)
      return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + (calib ? " has a kind that is none of BETWEEN, PRIOR, POINT and HANDEYE" : " has a kind that is none of BETWEEN, PRIOR and POINT"));
    if (i < 0 || j < 0 || i >= n_nodes || j >= n_nodes) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + " names a node out of range");
    int read = 6;
    if (kind == SMHIP_POSE_GRAPH_FACTOR_PRIOR) {
      if (i != j) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + " is a prior whose j is not its i");
      if (const char* p = transform_problem(dat)) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + "'s prior pose " + p);
    } else if (kind == SMHIP_POSE_GRAPH_FACTOR_POINT) {
      if (i == j) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + " is a point factor that joins a node to itself");
      for (int c = 0; c < 6; ++c)
        if (!std::isfinite(dat[c])) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + " has a lever arm or a point that is not finite");
      read = 3;
    } else if (handeye) {
      if (i == j) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + " is a hand-eye factor that joins a node to itself");
      if (const char* p = transform_problem(dat)) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + "'s odometer pose " + p);
    } else {
      if (i == j) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + " joins a node to itself");
      if (const char* p = transform_problem(dat)) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + "'s measurement " + p);
    }
    if (sigmas) {
      for (int c = 0; c < read; ++c) {
        const double s = sigmas[6 * (size_t)e + c];
        if (!std::isfinite(s) || !(s > 0.0)) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + " has a sigma that is not finite and positive");
      }
    } else if (kind != SMHIP_POSE_GRAPH_FACTOR_BETWEEN) {
      return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + " is no BETWEEN and needs its sigmas: the defaults are those of a BETWEEN");
    }
    ++degree[i];
    if (kind == SMHIP_POSE_GRAPH_FACTOR_PRIOR) { held[i] = 1; prior[i] = 1; continue; }       // listed once, diagonal: never a chain or non-chain edge
    ++degree[j];
    if (kind == SMHIP_POSE_GRAPH_FACTOR_BETWEEN) { held[i] = 1; held[j] = 1; }
    if (handeye) { held[i] = 1; calibrated[j] = 1; }                             // Ad(T^-1) is invertible: node i's block has full rank; B can vanish
    parent[root(i)] = root(j);
    if (i - j != 1 && j - i != 1) ++non_chain;
  }
  std::vector<uint8_t> anchored((size_t)n_nodes, 0);
  for (int k = 0; k < n_nodes; ++k) {
    if (!fixed[k] && degree[k] == 0) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "free node " + std::to_string(k) + " has no edge");
    if (!fixed[k] && calibrated[k] && !prior[k])
      return refuse(SMHIP_ERR_INVALID_ARGUMENT, "free node " + std::to_string(k) + " is the calibration node of a hand-eye factor and has no prior: the factor's B vanishes at h = I and is rank-deficient for planar motion");
    if (!fixed[k] && !held[k])
      return refuse(SMHIP_ERR_INVALID_ARGUMENT, "free node " + std::to_string(k) + " has point factors only, which leave its block at rank 3");
    if (fixed[k] || prior[k]) anchored[root(k)] = 1;
  }
  for (int k = 0; k < n_nodes; ++k)
    if (!anchored[root(k)]) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "the component of node " + std::to_string(k) + " has no fixed node" + (kinds ? " and no prior" : ""));
  if (plan) {
    plan->csr_offsets.assign((size_t)n_nodes + 1, 0);
    for (int k = 0; k < n_nodes; ++k) plan->csr_offsets[k + 1] = plan->csr_offsets[k] + degree[k];
    plan->csr_edges.assign((size_t)plan->csr_offsets[n_nodes], 0);
    std::vector<int32_t> at(plan->csr_offsets.begin(), plan->csr_offsets.end() - 1);
    for (int e = 0; e < n_factors; ++e) {                                     // ascending e: every node's list comes out sorted
      plan->csr_edges[at[ij[2 * e]]++] = e;
      if (ij[2 * e + 1] != ij[2 * e]) plan->csr_edges[at[ij[2 * e + 1]]++] = e;      // (a PRIOR once)
    }
    plan->non_chain_edges = non_chain;
    plan->pcg_cap = 12 * non_chain + 64;
    plan->levels = 0;
    while ((1 << plan->levels) < n_nodes) ++plan->levels;
  }
  return SMHIP_OK;
}

inline smhip_status check_and_plan_factors(int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds, const int32_t* ij,
                                           const double* data, const double* sigmas, Plan* plan, std::string* why) {
  return check_and_plan_kinds(false, n_nodes, poses, fixed, n_factors, kinds, ij, data, sigmas, plan, why);
}

// check_and_plan_kinds, then the Huber thresholds (one per factor, nullptr = none): each finite and not negative
inline smhip_status check_and_plan_calib(bool calib, int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds, const int32_t* ij,
                                         const double* data, const double* sigmas, const double* huber, Plan* plan, std::string* why) {
  Plan made;
  if (const smhip_status s = check_and_plan_kinds(calib, n_nodes, poses, fixed, n_factors, kinds, ij, data, sigmas, &made, why)) return s;
  for (int e = 0; huber && e < n_factors; ++e)
    if (!std::isfinite(huber[e]) || huber[e] < 0.0) {
      if (why) *why = "pose graph: edge " + std::to_string(e) + " has a Huber threshold that is negative or not finite";
      return SMHIP_ERR_INVALID_ARGUMENT;
    }
  if (plan) *plan = made;
  return SMHIP_OK;
}

// nullptr, or what is wrong with a row-major 6x6 square-root information: a non-finite entry, or singular -- the smallest pivot of
// an LU with partial pivoting at or below 1e-12 times the largest entry
inline const char* sqrt_info_problem(const double* L) {
  double a[36], big = 0.0;
  for (int k = 0; k < 36; ++k) {
    if (!std::isfinite(L[k])) return "has an entry that is not finite";
    a[k] = L[k];
    big = std::fmax(big, std::fabs(L[k]));
  }
  for (int c = 0; c < 6; ++c) {
    int p = c;
    for (int r = c + 1; r < 6; ++r) if (std::fabs(a[6 * r + c]) > std::fabs(a[6 * p + c])) p = r;
    if (p != c) for (int k = 0; k < 6; ++k) { const double t = a[6 * c + k]; a[6 * c + k] = a[6 * p + k]; a[6 * p + k] = t; }
    const double piv = a[6 * c + c];
    if (!(std::fabs(piv) > 1.0e-12 * big)) return "is singular";
    for (int r = c + 1; r < 6; ++r) {
      const double f = a[6 * r + c] / piv;
      for (int k = c; k < 6; ++k) a[6 * r + k] -= f * a[6 * c + k];
    }
  }
  return nullptr;
}

// check_and_plan_calib(true, ...), then the square-root informations: info_index one per factor (-1 = its sigmas, else an entry of
// sqrt_info: 36 doubles, row-major; an entry's index is below the factor count), nullptr = none.  *n_info: entries read.
inline smhip_status check_and_plan_info(int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds, const int32_t* ij,
                                        const double* data, const double* sigmas, const double* huber, const int32_t* info_index, const double* sqrt_info,
                                        Plan* plan, int* n_info, std::string* why) {
  Plan made;
  if (const smhip_status s = check_and_plan_calib(true, n_nodes, poses, fixed, n_factors, kinds, ij, data, sigmas, huber, &made, why)) return s;
  auto refuse = [&](const std::string& text) { if (why) *why = "pose graph: " + text; return SMHIP_ERR_INVALID_ARGUMENT; };
  int entries = 0;
  for (int e = 0; info_index && e < n_factors; ++e) {
    const int at = info_index[e];
    if (at == -1) continue;
    const std::string name = "edge " + std::to_string(e);
    if (at < -1 || at >= n_factors) return refuse(name + " has a square-root information index out of range");
    if (!sqrt_info) return refuse("null pointer");
    if ((kinds ? kinds[e] : SMHIP_POSE_GRAPH_FACTOR_BETWEEN) != SMHIP_POSE_GRAPH_FACTOR_BETWEEN)
      return refuse(name + " carries a square-root information and is no BETWEEN");
    if (const char* p = sqrt_info_problem(sqrt_info + 36 * (size_t)at)) return refuse(name + "'s square-root information " + p);
    entries = at + 1 > entries ? at + 1 : entries;
  }
  if (plan) *plan = made;
  if (n_info) *n_info = entries;
  return SMHIP_OK;
}

constexpr int kMargWorkgroupsPerCu = 4;                    // max_workgroups is clamped to this many per CU
constexpr long long kMargMaxOutputDoubles = 1LL << 27;     // cov and blocks of one call: 1 GiB

// What smhip_pose_graph_marginals decides before anything is touched.  last_n: the node count of the handle's last optimise call, -1 =
// none reached its launch; last_numeric: that call ended NUMERIC; pcg_cap: its cap; cus: the device's CU count.  SMHIP_OK and the grid
// in *workgroups, or the refusal with its reason in *why.  The budget is decided from the sizes alone: a workgroup runs
// ceil(n_query / G) queries of six solves of at most pcg_cap iterations one after the other.
inline smhip_status check_marginals(int last_n, bool last_numeric, int pcg_cap, int cus, int n_nodes, int n_query, const int32_t* query, const double* cov,
                                    int n_rows, const int32_t* rows, const double* blocks, int max_workgroups, int* workgroups, std::string* why) {
  auto refuse = [&](smhip_status s, const std::string& text) { if (why) *why = "pose graph marginals: " + text; return s; };
  if (last_n < 0) return refuse(SMHIP_ERR_NOT_READY, "no optimisation has been launched on this handle");
  if (last_numeric) return refuse(SMHIP_ERR_NOT_READY, "the last optimisation ended NUMERIC: there are no poses to linearise at");
  if (n_nodes != last_n) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "the last optimisation had " + std::to_string(last_n) + " nodes, not " + std::to_string(n_nodes));
  if (n_query < 1) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "at least one query");
  if (!query || !cov) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "null pointer");
  if (n_rows < 0 || (n_rows > 0 && (!rows || !blocks))) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "rows given without rows or blocks to write");
  if (max_workgroups < 0) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "max_workgroups is negative");
  for (int q = 0; q < n_query; ++q)
    if (query[q] < 0 || query[q] >= n_nodes) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "query " + std::to_string(q) + " names a node out of range");
  for (int r = 0; r < n_rows; ++r)
    if (rows[r] < 0 || rows[r] >= n_nodes) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "row " + std::to_string(r) + " names a node out of range");
  // More workgroups than a few per CU buy nothing (one of 1024 threads fills a CU) and each costs a slice of the workspace: clamped.
  const int most = kMargWorkgroupsPerCu * (cus > 0 ? cus : 1);
  int G = max_workgroups > 0 ? max_workgroups : (cus > 0 ? cus : 1);
  if (G > most) G = most;
  if (G > n_query) G = n_query;
  if (36.0 * n_query * (1.0 + n_rows) > (double)kMargMaxOutputDoubles)
    return refuse(SMHIP_ERR_CAPACITY, "cov and blocks together are more than " + std::to_string(kMargMaxOutputDoubles) + " doubles: ask for fewer nodes or rows per call");
  const long long rounds = ((long long)n_query + G - 1) / G;
  if (rounds * 6 * (long long)pcg_cap > SMHIP_POSE_GRAPH_MAX_PCG_TOTAL)
    return refuse(SMHIP_ERR_CAPACITY, std::to_string(rounds) + " queries per workgroup x 6 x the cap of " + std::to_string(pcg_cap) + " iterations is more than " +
                                          std::to_string(SMHIP_POSE_GRAPH_MAX_PCG_TOTAL) + ": ask for fewer nodes per call");
  if (workgroups) *workgroups = G;
  return SMHIP_OK;
}

inline smhip_status check_and_plan_robust(int n_nodes, const double* poses, const uint8_t* fixed, int n_factors, const uint8_t* kinds, const int32_t* ij,
                                          const double* data, const double* sigmas, const double* huber, Plan* plan, std::string* why) {
  return check_and_plan_calib(false, n_nodes, poses, fixed, n_factors, kinds, ij, data, sigmas, huber, plan, why);
}

inline smhip_status check_and_plan(int n_nodes, const double* poses, const uint8_t* fixed, int n_edges, const int32_t* edge_ij, const double* edge_Z,
                                   const double* edge_sigmas, Plan* plan, std::string* why) {
  return check_and_plan_factors(n_nodes, poses, fixed, n_edges, nullptr, edge_ij, edge_Z, edge_sigmas, plan, why);
}

}  // namespace pose_graph
}  // namespace smhip
