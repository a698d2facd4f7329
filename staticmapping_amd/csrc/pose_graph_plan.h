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
  std::vector<int32_t> csr_edges;        // 2 n_edges: the edges of node k, ascending, at [csr_offsets[k], csr_offsets[k + 1])
  int non_chain_edges = 0;               // |i - j| != 1
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

// SMHIP_OK and the plan, or the refusal with its reason in *why.  Reads nothing beyond the sizes it has accepted.
inline smhip_status check_and_plan(int n_nodes, const double* poses, const uint8_t* fixed, int n_edges, const int32_t* edge_ij, const double* edge_Z,
                                   const double* edge_sigmas, Plan* plan, std::string* why) {
  auto refuse = [&](smhip_status s, const std::string& text) { if (why) *why = "pose graph: " + text; return s; };
  if (!poses || !fixed || (n_edges > 0 && (!edge_ij || !edge_Z))) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "null pointer");
  if (n_nodes < 1 || n_edges < 0) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "at least one node and no negative edge count");
  if (n_nodes > kMaxNodes) return refuse(SMHIP_ERR_CAPACITY, "more than " + std::to_string(kMaxNodes) + " nodes");
  if (n_edges > kMaxEdges) return refuse(SMHIP_ERR_CAPACITY, "more than " + std::to_string(kMaxEdges) + " edges");
  for (int k = 0; k < n_nodes; ++k)
    if (const char* p = transform_problem(poses + 16 * (size_t)k)) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "pose " + std::to_string(k) + " " + p);
  std::vector<int32_t> parent((size_t)n_nodes), degree((size_t)n_nodes, 0);
  std::iota(parent.begin(), parent.end(), 0);
  auto root = [&](int a) { while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; } return a; };
  int non_chain = 0;
  for (int e = 0; e < n_edges; ++e) {
    const int i = edge_ij[2 * e], j = edge_ij[2 * e + 1];
    const std::string name = "edge " + std::to_string(e);
    if (i < 0 || j < 0 || i >= n_nodes || j >= n_nodes) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + " names a node out of range");
    if (i == j) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + " joins a node to itself");
    if (const char* p = transform_problem(edge_Z + 16 * (size_t)e)) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + "'s measurement " + p);
    if (edge_sigmas)
      for (int c = 0; c < 6; ++c) {
        const double s = edge_sigmas[6 * (size_t)e + c];
        if (!std::isfinite(s) || !(s > 0.0)) return refuse(SMHIP_ERR_INVALID_ARGUMENT, name + " has a sigma that is not finite and positive");
      }
    ++degree[i]; ++degree[j];
    parent[root(i)] = root(j);
    if (i - j != 1 && j - i != 1) ++non_chain;
  }
  std::vector<uint8_t> anchored((size_t)n_nodes, 0);
  for (int k = 0; k < n_nodes; ++k) {
    if (!fixed[k] && degree[k] == 0) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "free node " + std::to_string(k) + " has no edge");
    if (fixed[k]) anchored[root(k)] = 1;
  }
  for (int k = 0; k < n_nodes; ++k)
    if (!anchored[root(k)]) return refuse(SMHIP_ERR_INVALID_ARGUMENT, "the component of node " + std::to_string(k) + " has no fixed node");
  if (plan) {
    plan->csr_offsets.assign((size_t)n_nodes + 1, 0);
    for (int k = 0; k < n_nodes; ++k) plan->csr_offsets[k + 1] = plan->csr_offsets[k] + degree[k];
    plan->csr_edges.assign(2 * (size_t)n_edges, 0);
    std::vector<int32_t> at(plan->csr_offsets.begin(), plan->csr_offsets.end() - 1);
    for (int e = 0; e < n_edges; ++e) {                                       // ascending e: every node's list comes out sorted
      plan->csr_edges[at[edge_ij[2 * e]]++] = e;
      plan->csr_edges[at[edge_ij[2 * e + 1]]++] = e;
    }
    plan->non_chain_edges = non_chain;
    plan->pcg_cap = 12 * non_chain + 64;
    plan->levels = 0;
    while ((1 << plan->levels) < n_nodes) ++plan->levels;
  }
  return SMHIP_OK;
}

}  // namespace pose_graph
}  // namespace smhip
