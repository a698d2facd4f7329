// The pose graph's marginal covariances without a device: the kernel header's own per-query routine (csrc/pose_graph_kernel.h,
// marginal_query) under HostCtx -- one thread, empty barriers -- and what smhip_pose_graph_marginals decides on the host
// (csrc/pose_graph_plan.h, check_marginals).  Stand-alone: it links nothing of the library, so it also builds with
// -fsanitize=address,undefined.
//   test_pose_graph_marginals host             the refusals (the NUMERIC flag among them), probe 3's NUMERIC ending, the dealing of
//                                              queries to workgroups: the same bits for every grid and for a node queried alone
//   test_pose_graph_marginals solve IN OUT     probe 3 at the poses in IN, then every query of IN (see Solve), results to OUT
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <string>
#include <vector>

#include "../../staticmapping_amd/csrc/pose_graph_kernel.h"
#include "../../staticmapping_amd/csrc/pose_graph_plan.h"

namespace pg = smhip::pose_graph;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct Problem {
  int n = 0, m = 0, pcg_cap = 0;
  std::vector<double> cur, Z, sinv, huber, sqrt_info;          // 12 n, 12 m, 6 m, m or empty, 36 per entry or empty
  std::vector<int32_t> fixed, ij, kind, info_index, csr_off, csr_edge;
  std::vector<double> shared, wgt;
  std::vector<int32_t> out_i;
  pg::Dev d;

  // the node -> factors list as the library makes it: ascending, a PRIOR once
  void Csr() {
    const size_t N = static_cast<size_t>(n), M = static_cast<size_t>(m);
    csr_off.assign(N + 1, 0);
    for (size_t e = 0; e < M; ++e) {
      ++csr_off[static_cast<size_t>(ij[2 * e]) + 1];
      if (ij[2 * e + 1] != ij[2 * e]) ++csr_off[static_cast<size_t>(ij[2 * e + 1]) + 1];
    }
    for (size_t k = 0; k < N; ++k) csr_off[k + 1] += csr_off[k];
    csr_edge.assign(static_cast<size_t>(csr_off[N]), 0);
    std::vector<int32_t> at(csr_off.begin(), csr_off.end() - 1);
    for (size_t e = 0; e < M; ++e) {
      csr_edge[static_cast<size_t>(at[static_cast<size_t>(ij[2 * e])]++)] = static_cast<int32_t>(e);
      if (ij[2 * e + 1] != ij[2 * e]) csr_edge[static_cast<size_t>(at[static_cast<size_t>(ij[2 * e + 1])]++)] = static_cast<int32_t>(e);
    }
  }

  // the shared arrays probe 3 fills; the vectors of the loop are left null: a read of them outside a slice would fault here
  void Bind() {
    const size_t N = static_cast<size_t>(n), M = static_cast<size_t>(m);
    Csr();
    shared.assign(N * (7 * 36 + 6) + M * (2 * 36 + 6), std::numeric_limits<double>::quiet_NaN());
    wgt.assign(M, 0.0);
    out_i.assign(pg::kOutInts, -1);
    double* p = shared.data();
    auto take = [&p](size_t c) { double* r = p; p += c; return r; };
    d = pg::Dev();
    d.n = n; d.m = m; d.pcg_cap = pcg_cap; d.probe = 3;
    d.cur = cur.data(); d.Z = Z.data(); d.sinv = sinv.data();
    d.fixed = fixed.data(); d.ij = ij.data(); d.csr_off = csr_off.data(); d.csr_edge = csr_edge.data();
    d.kind = kind.empty() ? nullptr : kind.data();
    d.huber = huber.empty() ? nullptr : huber.data();
    d.info_index = info_index.empty() ? nullptr : info_index.data();
    d.sqrt_info = sqrt_info.empty() ? nullptr : sqrt_info.data();
    d.wgt = wgt.data();
    d.Hkk = take(36 * N); d.C = take(36 * N); d.D = take(36 * N); d.U = take(36 * N); d.Dinv = take(36 * N); d.Wm = take(36 * N); d.Wp = take(36 * N);
    d.g = take(6 * N);                                            // (assemble writes the shared g; the solves use their slice's)
    d.A = take(36 * M); d.B = take(36 * M); d.rw = take(6 * M);
    d.out_i = out_i.data();
  }

  bool Factor() {
    pg::HostCtx c;
    pg::run(d, c);
    return out_i[pg::kOutStop] == 0;
  }

  // the call's queries dealt to G "workgroups", each with its own slice, run one after the other
  void Query(int G, const std::vector<int32_t>& query, const std::vector<int32_t>& rows, std::vector<double>* cov, std::vector<double>* blocks,
             std::vector<int32_t>* info) const {
    const size_t Q = query.size(), R = rows.size();
    const size_t stride = static_cast<size_t>(pg::kMargNodeDoubles) * static_cast<size_t>(n) + static_cast<size_t>(pg::kMargEdgeDoubles) * static_cast<size_t>(m);
    std::vector<double> ws(stride * static_cast<size_t>(G), std::numeric_limits<double>::quiet_NaN());
    cov->assign(36 * Q, std::numeric_limits<double>::quiet_NaN());
    blocks->assign(36 * Q * R, std::numeric_limits<double>::quiet_NaN());
    info->assign(pg::kMargInts * Q, -1);
    for (int w = 0; w < G; ++w) {
      pg::Dev mine = d;
      pg::marginal_slice(&mine, ws.data() + stride * static_cast<size_t>(w));
      pg::HostCtx c;
      pg::marginal_queries(mine, c, w, G, static_cast<int>(Q), query.data(), static_cast<int>(R), rows.data(), cov->data(), R ? blocks->data() : nullptr, info->data());
    }
  }
};

// IN: int32 n, m, n_query, n_rows, pcg_cap, G, has_kind, has_huber, n_info (-1: no information arrays); doubles cur[12 n], Z[12 m],
// sinv[6 m], huber[m] if has_huber, sqrt_info[36 n_info] if n_info > 0; int32 fixed[n], ij[2 m], kind[m] if has_kind, info_index[m] if
// n_info >= 0, query[n_query], rows[n_rows].  OUT: doubles: 1 if the factorisation succeeded else 0, then cov[36 Q], blocks[36 Q R],
// info[3 Q] (as doubles).
static int Solve(const char* in_path, const char* out_path) {
  std::ifstream in(in_path, std::ios::binary);
  int32_t head[9];
  if (!in.read(reinterpret_cast<char*>(head), sizeof(head))) return 2;
  Problem p;
  p.n = head[0]; p.m = head[1]; p.pcg_cap = head[4];
  const int n_query = head[2], n_rows = head[3], G = head[5], has_kind = head[6], has_huber = head[7], n_info = head[8];
  if (p.n < 1 || p.m < 0 || n_query < 1 || n_rows < 0 || G < 1) return 2;
  const size_t N = static_cast<size_t>(p.n), M = static_cast<size_t>(p.m);
  auto rd = [&in](void* q, size_t bytes) { return bytes == 0 || static_cast<bool>(in.read(reinterpret_cast<char*>(q), static_cast<std::streamsize>(bytes))); };
  p.cur.resize(12 * N); p.Z.resize(12 * M); p.sinv.resize(6 * M); p.fixed.resize(N); p.ij.resize(2 * M);
  if (has_huber) p.huber.resize(M);
  if (n_info > 0) p.sqrt_info.resize(36 * static_cast<size_t>(n_info));
  if (has_kind) p.kind.resize(M);
  if (n_info >= 0) p.info_index.resize(M);
  std::vector<int32_t> query(static_cast<size_t>(n_query)), rows(static_cast<size_t>(n_rows));
  if (!rd(p.cur.data(), 96 * N) || !rd(p.Z.data(), 96 * M) || !rd(p.sinv.data(), 48 * M) || !rd(p.huber.data(), 8 * p.huber.size()) ||
      !rd(p.sqrt_info.data(), 8 * p.sqrt_info.size()) || !rd(p.fixed.data(), 4 * N) || !rd(p.ij.data(), 8 * M) || !rd(p.kind.data(), 4 * p.kind.size()) ||
      !rd(p.info_index.data(), 4 * p.info_index.size()) || !rd(query.data(), 4 * query.size()) || !rd(rows.data(), 4 * rows.size()))
    return 2;
  for (int32_t k : query) if (k < 0 || k >= p.n) return 2;
  for (int32_t k : rows) if (k < 0 || k >= p.n) return 2;
  for (size_t e = 0; e < 2 * M; ++e) if (p.ij[e] < 0 || p.ij[e] >= p.n) return 2;
  p.Bind();
  const double ok = p.Factor() ? 1.0 : 0.0;
  std::vector<double> cov, blocks;
  std::vector<int32_t> info;
  if (ok != 0.0) p.Query(G, query, rows, &cov, &blocks, &info);
  std::ofstream out(out_path, std::ios::binary);
  auto wr = [&out](const void* q, size_t bytes) { out.write(reinterpret_cast<const char*>(q), static_cast<std::streamsize>(bytes)); };
  wr(&ok, 8);
  wr(cov.data(), 8 * cov.size());
  wr(blocks.data(), 8 * blocks.size());
  std::vector<double> oi(info.begin(), info.end());
  wr(oi.data(), 8 * oi.size());
  return out ? 0 : 2;
}

// ---- host checks ---------------------------------------------------------------------------------------------------------------

// a ring of n nodes 2 m apart with one loop edge (2, n - 1) -- between free nodes, so that M is not all of H -- node 0 held, every pose a
// little off its measurement
static Problem Ring(int n) {
  Problem p;
  p.n = n; p.m = n;
  const size_t N = static_cast<size_t>(n);
  p.cur.resize(12 * N); p.Z.resize(12 * N); p.sinv.resize(6 * N); p.fixed.assign(N, 0); p.ij.resize(2 * N);
  p.fixed[0] = 1;
  auto pose = [](double x, double y, double yaw, double* o) {
    const double c = std::cos(yaw), s = std::sin(yaw);
    const double v[12] = {c, -s, 0, s, c, 0, 0, 0, 1, x, y, 0.1 * x};
    std::memcpy(o, v, sizeof(v));
  };
  for (int k = 0; k < n; ++k) {
    const double a = 2.0 * 3.14159265358979323846 * k / n, r = n / 3.14159265358979323846;
    pose(r * std::cos(a) + 0.01 * std::sin(7.0 * k), r * std::sin(a), a + 1.6 + 0.002 * std::cos(3.0 * k), &p.cur[12 * static_cast<size_t>(k)]);
    const size_t e = static_cast<size_t>(k);
    p.ij[2 * e] = k == n - 1 ? 2 : k; p.ij[2 * e + 1] = k == n - 1 ? n - 1 : k + 1;
    for (int c = 0; c < 6; ++c) p.sinv[6 * e + static_cast<size_t>(c)] = 1.0 / (c < 3 ? 0.1 : 0.15);
  }
  for (int e = 0; e < n; ++e) {                                    // Z = X_i^-1 X_j of the unperturbed ring
    const int i = p.ij[2 * static_cast<size_t>(e)], j = p.ij[2 * static_cast<size_t>(e) + 1];
    const double ai = 2.0 * 3.14159265358979323846 * i / n, aj = 2.0 * 3.14159265358979323846 * j / n, r = n / 3.14159265358979323846;
    double Xi[12], Xj[12];
    pose(r * std::cos(ai), r * std::sin(ai), ai + 1.6, Xi);
    pose(r * std::cos(aj), r * std::sin(aj), aj + 1.6, Xj);
    double* z = &p.Z[12 * static_cast<size_t>(e)];
    const double dt[3] = {Xj[9] - Xi[9], Xj[10] - Xi[10], Xj[11] - Xi[11]};
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b < 3; ++b) z[3 * a + b] = Xi[a] * Xj[b] + Xi[3 + a] * Xj[3 + b] + Xi[6 + a] * Xj[6 + b];
      z[9 + a] = Xi[a] * dt[0] + Xi[3 + a] * dt[1] + Xi[6 + a] * dt[2];
    }
  }
  p.pcg_cap = 12 * 1 + 64;
  p.Bind();
  return p;
}

static void RefusalChecks() {
  const int32_t query[3] = {1, 2, 1}, rows[2] = {0, 3};
  double cov[108], blocks[216];
  int G = -1;
  std::string why;
  auto call = [&](int last_n, bool numeric, int cap, int cus, int n_nodes, int n_query, const int32_t* q, const double* c, int n_rows, const int32_t* r,
                  const double* b, int max_wg) {
    why.clear(); G = -1;
    return pg::check_marginals(last_n, numeric, cap, cus, n_nodes, n_query, q, c, n_rows, r, b, max_wg, &G, &why);
  };
  EXPECT(call(4, false, 64, 256, 4, 3, query, cov, 2, rows, blocks, 0) == SMHIP_OK && G == 3);                 // min(n_query, CUs)
  EXPECT(call(4, false, 64, 256, 4, 3, query, cov, 0, nullptr, nullptr, 2) == SMHIP_OK && G == 2);
  EXPECT(call(4, false, 64, 2, 4, 3, query, cov, 0, nullptr, nullptr, 0) == SMHIP_OK && G == 2);
  EXPECT(call(-1, false, 64, 256, 4, 3, query, cov, 0, nullptr, nullptr, 0) == SMHIP_ERR_NOT_READY && !why.empty() && G == -1);
  EXPECT(call(4, true, 64, 256, 4, 3, query, cov, 0, nullptr, nullptr, 0) == SMHIP_ERR_NOT_READY && why.find("NUMERIC") != std::string::npos);   // the state's flag
  EXPECT(call(-1, true, 64, 256, 4, 0, nullptr, nullptr, 0, nullptr, nullptr, -1) == SMHIP_ERR_NOT_READY);     // NOT_READY comes first
  EXPECT(call(4, false, 64, 256, 5, 3, query, cov, 0, nullptr, nullptr, 0) == SMHIP_ERR_INVALID_ARGUMENT);
  EXPECT(call(4, false, 64, 256, 4, 0, query, cov, 0, nullptr, nullptr, 0) == SMHIP_ERR_INVALID_ARGUMENT);
  EXPECT(call(4, false, 64, 256, 4, 3, nullptr, cov, 0, nullptr, nullptr, 0) == SMHIP_ERR_INVALID_ARGUMENT);
  EXPECT(call(4, false, 64, 256, 4, 3, query, nullptr, 0, nullptr, nullptr, 0) == SMHIP_ERR_INVALID_ARGUMENT);
  EXPECT(call(4, false, 64, 256, 4, 3, query, cov, 2, nullptr, blocks, 0) == SMHIP_ERR_INVALID_ARGUMENT);
  EXPECT(call(4, false, 64, 256, 4, 3, query, cov, 2, rows, nullptr, 0) == SMHIP_ERR_INVALID_ARGUMENT);
  EXPECT(call(4, false, 64, 256, 4, 3, query, cov, -1, rows, blocks, 0) == SMHIP_ERR_INVALID_ARGUMENT);
  EXPECT(call(4, false, 64, 256, 4, 3, query, cov, 0, nullptr, nullptr, -1) == SMHIP_ERR_INVALID_ARGUMENT);
  EXPECT(call(2, false, 64, 256, 2, 3, query, cov, 0, nullptr, nullptr, 0) == SMHIP_ERR_INVALID_ARGUMENT);     // query 2 out of range
  EXPECT(call(3, false, 64, 256, 3, 3, query, cov, 2, rows, blocks, 0) == SMHIP_ERR_INVALID_ARGUMENT);         // row 3 out of range
  const int32_t negative[1] = {-1};
  EXPECT(call(4, false, 64, 256, 4, 1, negative, cov, 0, nullptr, nullptr, 0) == SMHIP_ERR_INVALID_ARGUMENT);
  // the budget, from the sizes alone: ceil(Q / G) x 6 x cap against SMHIP_POSE_GRAPH_MAX_PCG_TOTAL = 200 000
  std::vector<int32_t> many(2000, 1);
  std::vector<double> room(36 * 2000);
  EXPECT(call(4, false, 100, 256, 4, 2000, many.data(), room.data(), 0, nullptr, nullptr, 6) == SMHIP_ERR_CAPACITY);             // ceil(2000 / 6) = 334, x 600 = 200 400
  EXPECT(call(4, false, 100, 256, 4, 2000, many.data(), room.data(), 0, nullptr, nullptr, 7) == SMHIP_OK);                       // 286 x 600 = 171 600
  EXPECT(call(4, false, 100, 256, 4, 2000, many.data(), room.data(), 0, nullptr, nullptr, 5) == SMHIP_ERR_CAPACITY && !why.empty());   // 400 x 600 = 240 000
  EXPECT(call(4, false, 33334, 256, 4, 1, many.data(), room.data(), 0, nullptr, nullptr, 0) == SMHIP_ERR_CAPACITY);              // one query, 6 x 33 334 = 200 004
  EXPECT(call(4, false, 33333, 256, 4, 1, many.data(), room.data(), 0, nullptr, nullptr, 0) == SMHIP_OK);
}

static void NumericCheck() {
  Problem p = Ring(6);
  EXPECT(p.Factor());
  for (int c = 0; c < 6; ++c) { p.sinv[6 * 2 + static_cast<size_t>(c)] = 0.0; p.sinv[6 * 3 + static_cast<size_t>(c)] = 0.0; }      // node 3's two edges weigh nothing: its block is zero
  p.out_i.assign(pg::kOutInts, -1);
  EXPECT(!p.Factor() && p.out_i[pg::kOutStop] == SMHIP_POSE_GRAPH_STOP_NUMERIC);
}

static void DealingChecks() {
  Problem p = Ring(9);
  EXPECT(p.Factor());
  const std::vector<int32_t> all = {0, 1, 2, 3, 4, 5, 6, 7, 8}, five = {7, 2, 2, 0, 5}, rows = {0, 4, 8};
  std::vector<double> cov1, blk1, cov2, blk2, cov3, blk3, one, oneb;
  std::vector<int32_t> i1, i2, i3, io;
  p.Query(1, all, rows, &cov1, &blk1, &i1);
  p.Query(2, all, rows, &cov2, &blk2, &i2);
  p.Query(9, all, rows, &cov3, &blk3, &i3);
  EXPECT(cov1 == cov2 && cov1 == cov3 && blk1 == blk2 && blk1 == blk3 && i1 == i2 && i1 == i3);
  for (double v : cov1) EXPECT(std::isfinite(v));
  for (double v : blk1) EXPECT(std::isfinite(v));
  for (int a = 0; a < 36; ++a) EXPECT(cov1[static_cast<size_t>(a)] == 0.0);                                   // the held node
  for (size_t q = 0; q < 9; ++q) for (int a = 0; a < 36; ++a) EXPECT(blk1[36 * (3 * q) + static_cast<size_t>(a)] == 0.0);   // the held row
  for (size_t q = 1; q < 9; ++q) {
    EXPECT(i1[3 * q + pg::kMargCapped] == 0 && i1[3 * q + pg::kMargPcgMax] >= 1 && i1[3 * q + pg::kMargPcgMax] < p.pcg_cap);
    for (int a = 0; a < 6; ++a) {
      EXPECT(cov1[36 * q + 7 * static_cast<size_t>(a)] > 0.0);
      for (int b = 0; b < 6; ++b) EXPECT(cov1[36 * q + static_cast<size_t>(6 * a + b)] == cov1[36 * q + static_cast<size_t>(6 * b + a)]);
    }
  }
  // n_query = 5 over two workgroups (the stride with a remainder), with a repeat and the held node among them
  p.Query(2, five, rows, &cov2, &blk2, &i2);
  for (size_t q = 0; q < 5; ++q) {
    const size_t k = static_cast<size_t>(five[q]);
    EXPECT(std::memcmp(&cov2[36 * q], &cov1[36 * k], 36 * 8) == 0 && std::memcmp(&blk2[108 * q], &blk1[108 * k], 108 * 8) == 0);
    p.Query(1, {five[q]}, rows, &one, &oneb, &io);                                                          // queried alone
    EXPECT(std::memcmp(one.data(), &cov1[36 * k], 36 * 8) == 0 && std::memcmp(oneb.data(), &blk1[108 * k], 108 * 8) == 0);
  }
  // a cap too small: the flag, whatever the iterations gave
  Problem q = Ring(9);
  q.pcg_cap = 2;
  q.Bind();
  EXPECT(q.Factor());
  q.Query(1, {4}, {}, &one, &oneb, &io);
  EXPECT(io[pg::kMargCapped] == 1 && io[pg::kMargPcgMax] == 2 && io[pg::kMargPcg] == 12);
  // a solve that ends below the cap without meeting the stop rule: a NaN in a factor's rows makes p^T H p "not positive" at once
  Problem bad = Ring(9);
  EXPECT(bad.Factor());
  bad.d.A[36 * 4] = std::numeric_limits<double>::quiet_NaN();
  bad.Query(1, {4}, {}, &one, &oneb, &io);
  EXPECT(io[pg::kMargCapped] == 1 && io[pg::kMargPcgMax] < bad.pcg_cap);
  bad.Query(1, {0}, {}, &one, &oneb, &io);                                                                  // (the held node runs no solve)
  EXPECT(io[pg::kMargCapped] == 0 && io[pg::kMargPcg] == 0);
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "host") {
    RefusalChecks();
    NumericCheck();
    DealingChecks();
    std::printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
  }
  if (mode == "solve" && argc == 4) return Solve(argv[2], argv[3]);
  std::fprintf(stderr, "usage: test_pose_graph_marginals host | solve IN OUT\n");
  return 2;
}
