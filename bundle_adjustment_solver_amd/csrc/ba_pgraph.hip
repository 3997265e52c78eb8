// ba_pgraph.hip — pose-graph optimisation (ba_pgraph_*, include/ba_hip.h):
// Levenberg-Marquardt over relative-pose factors alone, chi2 = sum_f r_f^T Omega_f r_f.  The
// reference project has no counterpart; the definition is the comment in include/ba_hip.h.
// Host code only.  The kernels are those of ba_graph_kernels.hip at Se3Graph (ba_graph_fn.h), with
// the factor arithmetic of ba_rel_fn.h; the host side is the graph driver of
// ba_graph.hip, which this graph shares with the Sim(3) one (ba_sim3.hip).  Here are the driver's
// description of an SE(3) graph (kPgSpec: the widths, the launchers) and the ba_pgraph_* entry
// points, which check their pointers, validate the caller's arrays (ba_pgraph_host.h) and call the
// driver: the solve, the robust kernels (ba_pgraph_set_robust; §6l), the covariance blocks and the
// gate (ba_pgraph_covariance / ba_pgraph_gate; §6m).
#include "ba_graph.h"

using ba::fail;

struct ba_pgraph : ba::GraphHost {};

namespace {

const ba::GraphSpec kPgSpec = {
    "ba_pgraph",
    6,   // W
    12,  // pose_doubles: T_jw and Z as [R row-major, t]
    ba::kRelVal,
    ba::kPgRec,
    ba::kPgFpb,
    ba::dense_poses_per_tile,
    ba::relative_pack_values,
    ba::pgraph_validate_values,
    ba::launch_graph_lin<ba::Se3Graph>,
    ba::launch_graph_lin_robust<ba::Se3Graph>,
    ba::launch_graph_assemble<ba::Se3Graph>,
    ba::launch_graph_assemble_robust<ba::Se3Graph>,
    ba::launch_graph_trial<ba::Se3Graph>,
    ba::launch_graph_cov_batch<ba::Se3Graph>,
};

}  // namespace

extern "C" {

int ba_pgraph_check(int n_pose, const double *T_jw12, const uint8_t *pose_fixed, int64_t n_rel,
                    const int32_t *rel_j, const int32_t *rel_k, const double *Z12, const double *Omega36) {
  std::string err;
  if (ba::pgraph_validate_host(n_pose, T_jw12, pose_fixed, n_rel, rel_j, rel_k, Z12, Omega36, &err))
    return fail("ba_pgraph_create: " + err);
  return 0;
}

int ba_pgraph_create(ba_pgraph **out, ba_handle *h, int n_pose, const double *T_jw12, const uint8_t *pose_fixed,
                     int64_t n_rel, const int32_t *rel_j, const int32_t *rel_k, const double *Z12,
                     const double *Omega36) {
  if (!out) return fail("ba_pgraph_create: null out pointer");
  *out = nullptr;
  if (ba_pgraph_check(n_pose, T_jw12, pose_fixed, n_rel, rel_j, rel_k, Z12, Omega36)) return -1;
  if (!h) return fail("ba_pgraph_create: null handle");
  ba_pgraph *g = new ba_pgraph();
  if (ba::graph_create(kPgSpec, g, h, n_pose, T_jw12, pose_fixed, n_rel, rel_j, rel_k, Z12, Omega36)) {
    delete g;
    return -1;
  }
  *out = g;
  return 0;
}

void ba_pgraph_destroy(ba_pgraph *g) {
  if (!g) return;
  ba::graph_destroy(g);
  delete g;
}

int ba_pgraph_update_values(ba_pgraph *g, const double *T_jw12, const double *Z12, const double *Omega36) {
  if (!g) return fail("ba_pgraph_update_values: null graph");
  return ba::graph_update_values(kPgSpec, g, T_jw12, Z12, Omega36);
}

int ba_pgraph_robust_check(int64_t n_rel, const int32_t *kind, const double *scale) {
  std::string err;
  if (ba::pgraph_robust_validate_host(n_rel, kind, scale, &err)) return fail("ba_pgraph_set_robust: " + err);
  return 0;
}

int ba_pgraph_set_robust(ba_pgraph *g, const int32_t *kind, const double *scale) {
  if (!g) return fail("ba_pgraph_set_robust: null graph");
  if (ba_pgraph_robust_check(g->F, kind, scale)) return -1;
  return ba::graph_set_robust(g, kind, scale);
}

int ba_pgraph_factor_report(ba_pgraph *g, double *s, double *w) {
  if (!g) return fail("ba_pgraph_factor_report: null graph");
  return ba::graph_factor_weights(kPgSpec, g, s, w);
}

int ba_pgraph_solve(ba_pgraph *g, const ba_options *opt, ba_iter_info *rows, int cap, int *n_iter, int *converged) {
  if (!g || !opt) return fail("ba_pgraph_solve: bad argument");
  if (cap < 0 || (cap > 0 && !rows)) return fail("ba_pgraph_solve: rows is NULL for cap > 0");
  return ba::graph_solve(kPgSpec, g, opt, rows, cap, n_iter, converged);
}

int ba_pgraph_get_poses(ba_pgraph *g, double *T_jw12) {
  if (!g || !T_jw12) return fail("ba_pgraph_get_poses: bad argument");
  return ba::graph_get_poses(kPgSpec, g, T_jw12);
}

int ba_pgraph_cost(ba_pgraph *g, double *chi2) {
  if (!g || !chi2) return fail("ba_pgraph_cost: bad argument");
  return ba::graph_cost(kPgSpec, g, chi2);
}

int ba_pgraph_get_system(ba_pgraph *g, double *H, double *g6N) {
  if (!g) return fail("ba_pgraph_get_system: null graph");
  return ba::graph_get_system(kPgSpec, g, H, g6N);
}

int ba_pgraph_info(ba_pgraph *g, int64_t out8[8]) {
  if (!g || !out8) return fail("ba_pgraph_info: bad argument");
  ba::graph_info(g, out8);
  return 0;
}

int ba_pgraph_cov_check(int n_pose, const uint8_t *pose_fixed, int n_pose_sel, const int32_t *pose_sel,
                        const double *cov_pose36, int64_t n_pair, const int32_t *pair_j, const int32_t *pair_k,
                        const double *cov_rel36, int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k,
                        const double *Z12, const double *Omega36, const double *d2) {
  std::string err;
  if (ba::pgraph_cov_validate_host(n_pose, pose_fixed, n_pose_sel, pose_sel, cov_pose36, n_pair, pair_j, pair_k,
                                   cov_rel36, n_cand, cand_j, cand_k, Z12, Omega36, d2, &err))
    return fail(err);
  return 0;
}

int ba_pgraph_covariance(ba_pgraph *g, int n_pose_sel, const int32_t *pose_sel, double *cov_pose36, int64_t n_pair,
                         const int32_t *pair_j, const int32_t *pair_k, double *cov_cross36, double *cov_rel36,
                         int64_t *dropped_pivots) {
  if (!g) return fail("ba_pgraph_covariance: null graph");
  if (ba_pgraph_cov_check(g->n_pose, g->fixed.data(), n_pose_sel, pose_sel, cov_pose36, n_pair, pair_j, pair_k,
                          cov_rel36, 0, nullptr, nullptr, nullptr, nullptr, nullptr))
    return -1;
  return ba::graph_covariance(kPgSpec, g, n_pose_sel, pose_sel, cov_pose36, n_pair, pair_j, pair_k, cov_cross36,
                              cov_rel36, dropped_pivots);
}

int ba_pgraph_gate(ba_pgraph *g, int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k, const double *Z12,
                   const double *Omega36, double *d2, double *r6, double *innov36, int64_t *dropped_pivots) {
  if (!g) return fail("ba_pgraph_gate: null graph");
  if (ba_pgraph_cov_check(g->n_pose, g->fixed.data(), 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, n_cand,
                          cand_j, cand_k, Z12, Omega36, d2))
    return -1;
  return ba::graph_gate(kPgSpec, g, n_cand, cand_j, cand_k, Z12, Omega36, d2, r6, innov36, dropped_pivots);
}

int ba_pgraph_cov_info(ba_pgraph *g, int64_t out4[4]) {
  if (!g || !out4) return fail("ba_pgraph_cov_info: bad argument");
  ba::graph_cov_info(g, out4);
  return 0;
}

int ba_pgraph_last_ms(ba_pgraph *g, double *ms) {
  if (!g || !ms) return fail("ba_pgraph_last_ms: bad argument");
  *ms = ba::graph_last_ms(g);
  return 0;
}

}  // extern "C"
