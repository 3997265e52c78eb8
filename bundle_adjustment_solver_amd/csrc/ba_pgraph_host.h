// ba_pgraph_host.h — host side of the pose-graph optimisation (ba_pgraph_*, ba_pgraph.hip;
// DESIGN.md §6k): validation of the caller's arrays, the per-pose and per-block factor
// lists and the tile adjacency of the dense image.  Plain C++ with no HIP call, so that it
// also builds into a stand-alone program under the host sanitizers
// (tools/pgraph_host_check.cpp, tools/pgraph_robust_host_check.cpp).  The lists, the robust rules
// and the covariance / gate validation serve the Sim(3) graph too (ba_sim3_host.h).  Internal.
#ifndef BA_PGRAPH_HOST_H_
#define BA_PGRAPH_HOST_H_

#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "ba_rel_host.h"

namespace ba {

// Everything ba_pgraph_check refuses: empty inputs, then the rules and the wording of
// ba_relative_check (*err names the factor), then an optimisable pose that no factor names
// (*err names the pose: its diagonal block would be zero).  pose_fixed may be null.
inline int pgraph_validate_host(int n_pose, const double *T_jw12, const uint8_t *pose_fixed, int64_t n_rel,
                                const int32_t *rel_j, const int32_t *rel_k, const double *Z12,
                                const double *Omega36, std::string *err) {
  auto bad = [&](const std::string &m) {
    *err = m;
    return -1;
  };
  if (n_pose <= 0) return bad("n_pose must be >= 1");
  if (n_rel <= 0) return bad("n_rel must be >= 1: a pose graph needs a factor");
  if (!T_jw12) return bad("null pose array");
  if (relative_validate_host(kRelPairs | kRelValues, n_pose, pose_fixed, n_rel, rel_j, rel_k, Z12, Omega36, err))
    return -1;
  for (int64_t e = 0; e < (int64_t)n_pose * 12; ++e)
    if (!std::isfinite(T_jw12[e])) return bad("T_jw is not finite (pose " + std::to_string(e / 12) + ")");
  std::vector<uint8_t> named((size_t)n_pose, 0);
  for (int64_t f = 0; f < n_rel; ++f) named[rel_j[f]] = named[rel_k[f]] = 1;
  for (int p = 0; p < n_pose; ++p)
    if (!(pose_fixed && pose_fixed[p]) && !named[p])
      return bad("pose " + std::to_string(p) + " is optimisable but no factor names it");
  return 0;
}

// The values of ba_pgraph_update_values: what ba_pgraph_check refuses about the poses and about
// the factor values, in its wording (any array may be null: not checked).
inline int pgraph_validate_values(int n_pose, const double *T_jw12, int64_t n_rel, const double *Z12,
                                  const double *Omega36, std::string *err) {
  auto bad = [&](const std::string &m) {
    *err = m;
    return -1;
  };
  for (int64_t e = 0; e < (int64_t)n_pose * 12 && T_jw12; ++e)
    if (!std::isfinite(T_jw12[e])) return bad("T_jw is not finite (pose " + std::to_string(e / 12) + ")");
  for (int64_t f = 0; f < n_rel && (Z12 || Omega36); ++f) {
    const std::string at = " (factor " + std::to_string(f) + ")";
    for (int e = 0; e < 12 && Z12; ++e)
      if (!std::isfinite(Z12[12 * f + e])) return bad("Z is not finite" + at);
    for (int e = 0; e < 36 && Omega36; ++e)
      if (!std::isfinite(Omega36[36 * f + e])) return bad("Omega is not finite" + at);
  }
  return 0;
}

// Everything ba_pgraph_robust_check refuses: a kind outside 0..3, and on a factor whose kind is
// not 0 a scale that is not finite or not positive (*err names the factor).  kind == nullptr
// clears every kernel and is accepted; the scale of a kind-0 factor is never read.
constexpr int kPgKinds = 4;  // 0 none, 1 Huber, 2 Cauchy, 3 Geman-McClure
inline int pgraph_robust_validate_host(int64_t n_rel, const int32_t *kind, const double *scale, std::string *err) {
  auto bad = [&](const std::string &m, int64_t f) {
    *err = m + " (factor " + std::to_string(f) + ")";
    return -1;
  };
  if (n_rel < 0) {
    *err = "n_rel must be >= 0";
    return -1;
  }
  if (!kind) return 0;
  for (int64_t f = 0; f < n_rel; ++f) {
    if (kind[f] < 0 || kind[f] >= kPgKinds) return bad("kind = " + std::to_string(kind[f]) + " is not one of 0..3", f);
    if (kind[f] == 0) continue;
    if (!scale) return bad("null scale array", f);
    if (!std::isfinite(scale[f])) return bad("scale is not finite", f);
    if (!(scale[f] > 0.0)) return bad("scale must be > 0", f);
  }
  return 0;
}

// The structure of a validated graph: the shared lists (ba_rel_host.h) plus the graph's own
// numbering.  The optimisable poses keep the user's order: optimisable index = rank among the
// optimisable poses.  A coupled block's key is hi * N + lo, so the blocks ascend in (hi, lo);
// H_jk is block (j, k): below the diagonal as it is when j > k, transposed otherwise.
struct PgraphLists : RelLists {
  int N = 0;
  std::vector<int32_t> opt_of_pose;   // per pose: optimisable index or -1
  std::vector<int32_t> opt_pose;      // per optimisable pose: its pose
  std::vector<int32_t> blk;           // 2 per coupled block: optimisable poses {hi, lo}, hi > lo
};

inline void pgraph_build_lists(int n_pose, const uint8_t *pose_fixed, int64_t n_rel, const int32_t *rel_j,
                               const int32_t *rel_k, PgraphLists *out) {
  PgraphLists &l = *out;
  l = PgraphLists();
  l.opt_of_pose.assign((size_t)n_pose, -1);
  for (int p = 0; p < n_pose; ++p)
    if (!(pose_fixed && pose_fixed[p])) {
      l.opt_of_pose[p] = l.N++;
      l.opt_pose.push_back(p);
    }
  const int64_t N = l.N;
  relative_build_lists(
      n_rel, rel_j, rel_k, l.N, l.opt_of_pose.data(),
      [N](int32_t a, int32_t b) { return std::pair<int64_t, bool>(std::max(a, b) * N + std::min(a, b), a < b); }, &l);
  for (int64_t key : l.bkey) {
    l.blk.push_back((int32_t)(key / N));
    l.blk.push_back((int32_t)(key % N));
  }
}

// Symmetric ncb x ncb tile adjacency (row-major bytes, zero diagonal) of the coupled blocks
// with poses_per_tile optimisable poses per tile, in the order of their indices.
inline void pgraph_tile_adjacency(const PgraphLists &l, int poses_per_tile, int *ncb, std::vector<uint8_t> *adj) {
  const int n = std::max(1, (l.N + poses_per_tile - 1) / poses_per_tile);
  *ncb = n;
  adj->assign((size_t)n * n, 0);
  for (size_t b = 0; b + 1 < l.blk.size(); b += 2) {
    const int I = l.blk[b] / poses_per_tile, J = l.blk[b + 1] / poses_per_tile;
    if (I != J) (*adj)[(size_t)I * n + J] = (*adj)[(size_t)J * n + I] = 1;
  }
}

// ---- covariance blocks and the chi-square gate (ba_pgraph_covariance / ba_pgraph_gate;
// ---- DESIGN.md §6m) -------------------------------------------------------------------------

// Cholesky of the W x W matrix (W <= 7) whose lower triangle is in O (row-major); false at a
// pivot that is not positive (or not finite).  The same loop as the device's (cholw of
// ba_graph_kernels.hip).
inline bool chol_host(const double *O, int W) {
  double L[49];
  for (int c = 0; c < W; ++c) {
    double d = O[c * W + c];
    for (int m = 0; m < c; ++m) d -= L[c * W + m] * L[c * W + m];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    const double s = std::sqrt(d);
    L[c * W + c] = s;
    for (int r = c + 1; r < W; ++r) {
      double v = O[r * W + c];
      for (int m = 0; m < c; ++m) v -= L[r * W + m] * L[c * W + m];
      L[r * W + c] = v / s;
    }
  }
  return true;
}

// The names a graph kind gives the covariance / gate validation: its two calls, its output arrays
// as the messages spell them, and the rules of its candidates: pairs and values, in the wording
// of a factor ("(factor 3)").
struct GraphCovNames {
  const char *covariance, *gate, *cov_pose, *cov_rel;
  int (*check_candidates)(int n_pose, const uint8_t *pose_fixed, int64_t n_cand, const int32_t *cand_j,
                          const int32_t *cand_k, const double *Z, const double *Omega, std::string *err);
};

// Everything ba_pgraph_cov_check and ba_sim3_cov_check refuse at tangent width W, in the order of
// the header's list; *err carries the call's name.  The pairs follow the pair rules of
// ba_relative_check, the candidates the kind's pair and value rules, in their wording ("(pair 3)",
// "(candidate 3)" for "(factor 3)"); then a candidate whose Omega is not positive definite.
inline int graph_cov_validate_host(int W, const GraphCovNames &names, int n_pose, const uint8_t *pose_fixed,
                                   int n_pose_sel, const int32_t *pose_sel, const double *cov_pose, int64_t n_pair,
                                   const int32_t *pair_j, const int32_t *pair_k, const double *cov_rel,
                                   int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k, const double *Z,
                                   const double *Omega, const double *d2, std::string *err) {
  const std::string cov = std::string(names.covariance) + ": ", gate = std::string(names.gate) + ": ";
  auto bad = [&](const std::string &m) {
    *err = m;
    return -1;
  };
  if (n_pose < 1) return bad(cov + "n_pose must be >= 1");
  if (n_pose_sel < 0 || n_pair < 0) return bad(cov + "negative selection size");
  if (n_cand < 0) return bad(gate + "negative number of candidates");
  if (n_pose_sel > 0 && !pose_sel) return bad(cov + "pose_sel is NULL for a non-empty selection");
  if (n_pose_sel > 0 && !cov_pose) return bad(cov + names.cov_pose + " is NULL for a non-empty pose selection");
  if (n_pair > 0 && !cov_rel) return bad(cov + names.cov_rel + " is NULL for a non-empty pair selection");
  if (n_cand > 0 && !d2) return bad(gate + "d2 is NULL for a non-empty candidate list");
  for (int s = 0; s < n_pose_sel; ++s) {
    const int u = pose_sel[s];
    if (u < 0 || u >= n_pose)
      return bad(cov + "pose_sel[" + std::to_string(s) + "] = " + std::to_string(u) + " is out of range");
    if (pose_fixed && pose_fixed[u])
      return bad(cov + "pose_sel[" + std::to_string(s) + "] = " + std::to_string(u) + " is a fixed pose");
  }
  // the shared validations say "factor"; here the entry is a pair or a candidate
  auto renamed = [&](const std::string &call, const char *entry) {
    const size_t at = err->rfind("factor ");
    if (at != std::string::npos) err->replace(at, 7, std::string(entry) + " ");
    *err = call + *err;
    return -1;
  };
  if (relative_validate_host(kRelPairs, n_pose, pose_fixed, n_pair, pair_j, pair_k, nullptr, nullptr, err))
    return renamed(cov, "pair");
  if (names.check_candidates(n_pose, pose_fixed, n_cand, cand_j, cand_k, Z, Omega, err))
    return renamed(gate, "candidate");
  for (int64_t c = 0; c < n_cand; ++c)
    if (!chol_host(Omega + (size_t)W * W * c, W))
      return bad(gate + "Omega is not positive definite (candidate " + std::to_string(c) + ")");
  return 0;
}

// The SE(3) graph's: the candidates follow the pair and the value rules of ba_relative_check
inline int pgraph_check_candidates(int n_pose, const uint8_t *pose_fixed, int64_t n_cand, const int32_t *cand_j,
                                   const int32_t *cand_k, const double *Z12, const double *Omega36,
                                   std::string *err) {
  return relative_validate_host(kRelPairs | kRelValues, n_pose, pose_fixed, n_cand, cand_j, cand_k, Z12, Omega36, err);
}
inline int pgraph_cov_validate_host(int n_pose, const uint8_t *pose_fixed, int n_pose_sel, const int32_t *pose_sel,
                                    const double *cov_pose36, int64_t n_pair, const int32_t *pair_j,
                                    const int32_t *pair_k, const double *cov_rel36, int64_t n_cand,
                                    const int32_t *cand_j, const int32_t *cand_k, const double *Z12,
                                    const double *Omega36, const double *d2, std::string *err) {
  const GraphCovNames names = {"ba_pgraph_covariance", "ba_pgraph_gate", "cov_pose36", "cov_rel36",
                               pgraph_check_candidates};
  return graph_cov_validate_host(6, names, n_pose, pose_fixed, n_pose_sel, pose_sel, cov_pose36, n_pair, pair_j,
                                 pair_k, cov_rel36, n_cand, cand_j, cand_k, Z12, Omega36, d2, err);
}

// One wave of k_graph_cov_solve owns 16 right-hand sides: the six identity columns of the pose
// opt[0] in its columns 0..5 and of opt[1] in 6..11 (optimisable indices; -1: no column, the
// blocks of that member are zero).  kind 0: two selected poses, slot[a] = row of the pose
// output; kind 1: the pair (j, k) = (pose[0], pose[1]), slot[0] = row of the pair outputs;
// kind 2: a candidate likewise.  t0 = tile position of the first non-zero row.
constexpr int kPgCovPoses = 0, kPgCovPair = 1, kPgCovCand = 2;
struct PgCovGroup {
  int32_t t0, kind;
  int32_t opt[2], slot[2], pose[2];
  int32_t pad_[8];
};
static_assert(sizeof(PgCovGroup) == 64, "PgCovGroup is one 64-byte record");

// The groups of one call on a validated selection, each kind ordered by the tile of its first
// non-zero row (ties: by column, then by input position): the distinct selected poses two per
// wave as ba_covariance groups them, then one wave per pair or candidate (entry_kind), repeats
// included.  pose_col: first image column per optimisable pose; nb: the tile order.
// slot_of_opt[optimisable index] = row of the pose output or -1; *n_pose_rows = rows of it.
inline void pgraph_cov_groups(const PgraphLists &l, const std::vector<int> &pose_col, int nb, int n_pose_sel,
                              const int32_t *pose_sel, int64_t n_entry, const int32_t *entry_j,
                              const int32_t *entry_k, int entry_kind, std::vector<PgCovGroup> *groups,
                              std::vector<int32_t> *slot_of_opt, int *n_pose_rows) {
  struct Item {
    int t0, col;
    int64_t idx;
  };
  auto less = [](const Item &a, const Item &b) {
    return a.t0 != b.t0 ? a.t0 < b.t0 : a.col != b.col ? a.col < b.col : a.idx < b.idx;
  };
  groups->clear();
  slot_of_opt->assign((size_t)l.N, -1);
  std::vector<Item> poses;
  for (int s = 0; s < n_pose_sel; ++s) {
    const int j = l.opt_of_pose[pose_sel[s]];
    poses.push_back({pose_col[j] / nb, pose_col[j], j});
  }
  std::sort(poses.begin(), poses.end(), less);
  poses.erase(std::unique(poses.begin(), poses.end(), [](const Item &a, const Item &b) { return a.idx == b.idx; }),
              poses.end());
  *n_pose_rows = (int)poses.size();
  for (size_t k = 0; k < poses.size(); k += 2) {
    PgCovGroup g{};
    g.kind = kPgCovPoses;
    g.t0 = poses[k].t0;
    for (int a = 0; a < 2; ++a) {
      const bool has = k + a < poses.size();
      g.opt[a] = has ? (int32_t)poses[k + a].idx : -1;
      g.slot[a] = has ? (int32_t)(k + a) : -1;
      g.pose[a] = has ? l.opt_pose[(size_t)poses[k + a].idx] : -1;
      if (has) (*slot_of_opt)[(size_t)poses[k + a].idx] = (int32_t)(k + a);
    }
    groups->push_back(g);
  }
  std::vector<Item> entries;
  for (int64_t p = 0; p < n_entry; ++p) {
    const int a = l.opt_of_pose[entry_j[p]], b = l.opt_of_pose[entry_k[p]];
    const int ca = a >= 0 ? pose_col[a] : INT32_MAX, cb = b >= 0 ? pose_col[b] : INT32_MAX;
    const int c0 = std::min(ca, cb);  // (validated: not both fixed)
    entries.push_back({c0 / nb, c0, p});
  }
  std::sort(entries.begin(), entries.end(), less);
  for (const Item &it : entries) {
    PgCovGroup g{};
    g.kind = entry_kind;
    g.t0 = it.t0;
    g.pose[0] = entry_j[it.idx];
    g.pose[1] = entry_k[it.idx];
    g.opt[0] = l.opt_of_pose[g.pose[0]];
    g.opt[1] = l.opt_of_pose[g.pose[1]];
    g.slot[0] = g.slot[1] = (int32_t)it.idx;
    groups->push_back(g);
  }
}

// Per tile position t of a schedule: the positions s < t with a structurally non-zero factor
// tile L(t, s), ascending (row_ptr / rows: per position its row tiles, the rhs block ncb among them).
inline void pgraph_cov_tile_rows(int ncb, const std::vector<int> &row_ptr, const std::vector<int> &rows,
                                 std::vector<int> *trow_ptr, std::vector<int> *trow) {
  std::vector<std::vector<int>> by_row((size_t)ncb);
  for (int p = 0; p < ncb; ++p)
    for (int a = row_ptr[p]; a < row_ptr[p + 1]; ++a)
      if (rows[a] < ncb) by_row[rows[a]].push_back(p);
  trow_ptr->assign((size_t)ncb + 1, 0);
  trow->clear();
  for (int t = 0; t < ncb; ++t) {
    trow->insert(trow->end(), by_row[t].begin(), by_row[t].end());
    (*trow_ptr)[t + 1] = (int)trow->size();
  }
}

}  // namespace ba
#endif  // BA_PGRAPH_HOST_H_
