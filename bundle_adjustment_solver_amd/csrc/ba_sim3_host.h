// ba_sim3_host.h — host side of the Sim(3) pose graph (ba_sim3_*, ba_sim3.hip):
// validation of the caller's arrays, the packing of the values the device reads, and the tile
// adjacency of the dense image at seven columns per pose.  The lists are the pose graph's
// (PgraphLists / pgraph_build_lists of ba_pgraph_host.h know nothing of a pose's width).
// Plain C++ with no HIP call, so that it also builds into a stand-alone program under the host
// sanitizers (tools/sim3_host_check.cpp).  Internal.
#ifndef BA_SIM3_HOST_H_
#define BA_SIM3_HOST_H_

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ba_dense_sched.h"
#include "ba_pgraph_host.h"

namespace ba {

// The values of the factors and the poses: what ba_sim3_check refuses about them, for
// ba_sim3_create and ba_sim3_update_values alike (either array may be null: not checked).
inline int sim3_validate_values(int n_pose, const double *S13, int64_t n_rel, const double *Z13,
                                const double *Omega49, std::string *err) {
  auto bad = [&](const std::string &m) {
    *err = m;
    return -1;
  };
  for (int64_t f = 0; f < n_rel && (Z13 || Omega49); ++f) {
    const std::string at = " (factor " + std::to_string(f) + ")";
    if (Z13) {
      const double *Z = Z13 + 13 * f;
      for (int e = 0; e < 9; ++e)
        if (!std::isfinite(Z[e])) return bad("the rotation of Z is not finite" + at);
      for (int e = 9; e < 12; ++e)
        if (!std::isfinite(Z[e])) return bad("Z is not finite" + at);
      if (!std::isfinite(Z[12])) return bad("the scale of Z is not finite" + at);
      if (!(Z[12] > 0.0)) return bad("the scale of Z must be > 0" + at);
    }
    if (Omega49)
      for (int e = 0; e < 49; ++e)
        if (!std::isfinite(Omega49[49 * f + e])) return bad("Omega is not finite" + at);
  }
  for (int p = 0; p < n_pose && S13; ++p) {
    const std::string at = " (pose " + std::to_string(p) + ")";
    const double *S = S13 + 13 * (size_t)p;
    for (int e = 0; e < 9; ++e)
      if (!std::isfinite(S[e])) return bad("the rotation of S_jw is not finite" + at);
    for (int e = 9; e < 12; ++e)
      if (!std::isfinite(S[e])) return bad("S_jw is not finite" + at);
    if (!std::isfinite(S[12])) return bad("the scale of S_jw is not finite" + at);
    if (!(S[12] > 0.0)) return bad("the scale of S_jw must be > 0" + at);
  }
  return 0;
}

// Everything ba_sim3_check refuses: the rules and the wording of ba_pgraph_check (empty inputs,
// the pair rules of ba_relative_check, non-finite values, an optimisable pose that no factor
// names), plus a scale that is not finite or not positive and a rotation that is not finite, of
// a pose or of Z.  pose_fixed may be null.
inline int sim3_validate_host(int n_pose, const double *S13, const uint8_t *pose_fixed, int64_t n_rel,
                              const int32_t *rel_j, const int32_t *rel_k, const double *Z13, const double *Omega49,
                              std::string *err) {
  auto bad = [&](const std::string &m) {
    *err = m;
    return -1;
  };
  if (n_pose <= 0) return bad("n_pose must be >= 1");
  if (n_rel <= 0) return bad("n_rel must be >= 1: a pose graph needs a factor");
  if (!S13) return bad("null pose array");
  if (!Z13 || !Omega49) return bad("null factor array (factor 0)");
  if (relative_validate_host(kRelPairs, n_pose, pose_fixed, n_rel, rel_j, rel_k, nullptr, nullptr, err)) return -1;
  if (sim3_validate_values(n_pose, S13, n_rel, Z13, Omega49, err)) return -1;
  std::vector<uint8_t> named((size_t)n_pose, 0);
  for (int64_t f = 0; f < n_rel; ++f) named[rel_j[f]] = named[rel_k[f]] = 1;
  for (int p = 0; p < n_pose; ++p)
    if (!(pose_fixed && pose_fixed[p]) && !named[p])
      return bad("pose " + std::to_string(p) + " is optimisable but no factor names it");
  return 0;
}

// The values of the factors as the device reads them: 62 doubles per factor, Z (13) and then
// Omega (49) with its lower triangle mirrored into the upper one.
constexpr int kS3Val = 62;
inline void sim3_pack_values(int64_t n_rel, const double *Z13, const double *Omega49, std::vector<double> *out) {
  out->resize((size_t)n_rel * kS3Val);
  for (int64_t f = 0; f < n_rel; ++f) {
    double *v = out->data() + (size_t)f * kS3Val;
    std::memcpy(v, Z13 + 13 * f, 13 * sizeof(double));
    const double *O = Omega49 + 49 * f;
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) v[13 + r * 7 + c] = r >= c ? O[r * 7 + c] : O[c * 7 + r];
  }
}

// Seven columns per pose: 4 poses (+ 4 padding columns) in a tile of order 32, 9 (+ 1) at 64.
// Beside dense_poses_per_tile (ba_dense_sched.h), which stays the six-column count.
inline int dense_sim3_per_tile(int nb) { return nb / 7; }

// The tile adjacency of the coupled blocks at that count
inline void sim3_tile_adjacency(const PgraphLists &l, int nb, int *ncb, std::vector<uint8_t> *adj) {
  pgraph_tile_adjacency(l, dense_sim3_per_tile(nb), ncb, adj);
}

// ---- covariance blocks and the chi-square gate (ba_sim3_covariance / ba_sim3_gate;
// ---- DESIGN.md §6p) -------------------------------------------------------------------------

// graph_cov_validate_host (ba_pgraph_host.h) at width 7.  The candidates follow the pair rules of
// ba_relative_check and the value rules of ba_sim3_check.
inline int sim3_check_candidates(int n_pose, const uint8_t *pose_fixed, int64_t n_cand, const int32_t *cand_j,
                                 const int32_t *cand_k, const double *Z13, const double *Omega49, std::string *err) {
  if (n_cand > 0 && (!Z13 || !Omega49)) {
    *err = "null factor array (factor 0)";
    return -1;
  }
  if (relative_validate_host(kRelPairs, n_pose, pose_fixed, n_cand, cand_j, cand_k, nullptr, nullptr, err)) return -1;
  return sim3_validate_values(0, nullptr, n_cand, Z13, Omega49, err);
}
inline int sim3_cov_validate_host(int n_pose, const uint8_t *pose_fixed, int n_pose_sel, const int32_t *pose_sel,
                                  const double *cov_pose49, int64_t n_pair, const int32_t *pair_j,
                                  const int32_t *pair_k, const double *cov_rel49, int64_t n_cand,
                                  const int32_t *cand_j, const int32_t *cand_k, const double *Z13,
                                  const double *Omega49, const double *d2, std::string *err) {
  const GraphCovNames names = {"ba_sim3_covariance", "ba_sim3_gate", "cov_pose49", "cov_rel49", sim3_check_candidates};
  return graph_cov_validate_host(7, names, n_pose, pose_fixed, n_pose_sel, pose_sel, cov_pose49, n_pair, pair_j,
                                 pair_k, cov_rel49, n_cand, cand_j, cand_k, Z13, Omega49, d2, err);
}

}  // namespace ba
#endif  // BA_SIM3_HOST_H_
