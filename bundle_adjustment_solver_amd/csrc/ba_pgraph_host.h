// ba_pgraph_host.h — host side of the pose-graph optimisation (ba_pgraph_*, ba_pgraph.hip;
// DESIGN.md §6k): validation of the caller's arrays, the per-pose and per-block factor
// lists and the tile adjacency of the dense image.  Plain C++ with no HIP call, so that it
// also builds into a stand-alone program under the host sanitizers
// (tools/pgraph_host_check.cpp, tools/pgraph_robust_host_check.cpp).  Internal.
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

}  // namespace ba
#endif  // BA_PGRAPH_HOST_H_
