// ba_sim3.hip — Sim(3) pose-graph optimisation (ba_sim3_*, include/ba_hip.h):
// Levenberg-Marquardt over relative-similarity factors alone, 7 DoF per pose, chi2 = sum_f
// r_f^T Omega_f r_f.  The 7-DoF loop closing of a monocular map; the reference project has no
// counterpart, the definition is the comment of ba_sim3_create.
// Host code only.  The kernels are those of ba_graph_kernels.hip at Sim3Graph (ba_graph_fn.h),
// with the factor arithmetic of ba_sim3_fn.h; the lists are the pose graph's (ba_pgraph_host.h),
// the linear solve is the level-scheduled tile Cholesky of ba_dense.hip with seven columns per
// pose; the host side is the graph driver of ba_graph.hip, which this graph shares with the SE(3)
// one (ba_pgraph.hip).  Here are the driver's description of a Sim(3) graph (kS3Spec: the widths,
// the launchers) and the ba_sim3_* entry points, which check their pointers, validate the caller's
// arrays (ba_sim3_host.h) and call the driver: the solve, the robust kernels (ba_sim3_set_robust;
// §6p), the covariance blocks and the gate (ba_sim3_covariance / ba_sim3_gate; §6p).
// ba_sim3_factor_report alone launches a kernel itself: the plain linearisation with an array for
// s_f.
#include "ba_graph.h"
#include "ba_sim3_host.h"
#include "ba_sim3_fn.h"

using ba::fail;

struct ba_sim3 : ba::GraphHost {
  double *rep = nullptr;  // s_f per factor of ba_sim3_factor_report (allocated by its first call)
};

namespace {

const ba::GraphSpec kS3Spec = {
    "ba_sim3",
    7,   // W
    13,  // pose_doubles: S_jw and Z as [R row-major, t, s]
    ba::kS3Val,
    ba::kS3Rec,
    ba::kS3Fpb,
    ba::dense_sim3_per_tile,
    ba::sim3_pack_values,
    ba::sim3_validate_values,
    ba::launch_graph_lin<ba::Sim3Graph>,
    ba::launch_graph_lin_robust<ba::Sim3Graph>,
    ba::launch_graph_assemble<ba::Sim3Graph>,
    ba::launch_graph_assemble_robust<ba::Sim3Graph>,
    ba::launch_graph_trial<ba::Sim3Graph>,
    ba::launch_graph_cov_batch<ba::Sim3Graph>,
};

}  // namespace

extern "C" {

void ba_sim3_exp(const double *xi7, double *S13) { ba::sim3_exp(xi7, S13); }
void ba_sim3_log(const double *S13, double *xi7) { ba::sim3_log(S13, xi7); }
void ba_sim3_adjoint(const double *S13, double *Ad49) { ba::sim3_Ad(S13, Ad49); }

int ba_sim3_check(int n_pose, const double *S13, const uint8_t *pose_fixed, int64_t n_rel, const int32_t *rel_j,
                  const int32_t *rel_k, const double *Z13, const double *Omega49) {
  std::string err;
  if (ba::sim3_validate_host(n_pose, S13, pose_fixed, n_rel, rel_j, rel_k, Z13, Omega49, &err))
    return fail("ba_sim3_create: " + err);
  return 0;
}

int ba_sim3_create(ba_sim3 **out, ba_handle *h, int n_pose, const double *S13, const uint8_t *pose_fixed,
                   int64_t n_rel, const int32_t *rel_j, const int32_t *rel_k, const double *Z13,
                   const double *Omega49) {
  if (!out) return fail("ba_sim3_create: null out pointer");
  *out = nullptr;
  if (ba_sim3_check(n_pose, S13, pose_fixed, n_rel, rel_j, rel_k, Z13, Omega49)) return -1;
  if (!h) return fail("ba_sim3_create: null handle");
  ba_sim3 *g = new ba_sim3();
  if (ba::graph_create(kS3Spec, g, h, n_pose, S13, pose_fixed, n_rel, rel_j, rel_k, Z13, Omega49)) {
    delete g;
    return -1;
  }
  *out = g;
  return 0;
}

void ba_sim3_destroy(ba_sim3 *g) {
  if (!g) return;
  ba::graph_destroy(g);
  delete g;
}

int ba_sim3_update_values(ba_sim3 *g, const double *S13, const double *Z13, const double *Omega49) {
  if (!g) return fail("ba_sim3_update_values: null graph");
  return ba::graph_update_values(kS3Spec, g, S13, Z13, Omega49);
}

int ba_sim3_factor_report(ba_sim3 *g, double *s) {
  if (!g || !s) return fail("ba_sim3_factor_report: bad argument");
  ba_handle *h = g->h;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (!g->rep) {
    const size_t mark = h->allocs.size();
    const int rc = h->dalloc(ba::Mem::Resident, &g->rep, (size_t)g->F);
    ba::graph_adopt_allocs(g, mark);
    if (rc) {
      g->rep = nullptr;
      return -1;
    }
    HIP_TRY(hipMemset(g->rep, 0, (size_t)g->F * sizeof(double)));
  }
  if (ba::graph_begin_pass(g)) return -1;
  ba::launch_s3_lin(g->d, 2, g->rep, h->stream);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(s, g->rep, (size_t)g->F * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int ba_sim3_robust_check(int64_t n_rel, const int32_t *kind, const double *scale) {
  std::string err;
  if (ba::pgraph_robust_validate_host(n_rel, kind, scale, &err)) return fail("ba_sim3_set_robust: " + err);
  return 0;
}

int ba_sim3_set_robust(ba_sim3 *g, const int32_t *kind, const double *scale) {
  if (!g) return fail("ba_sim3_set_robust: null graph");
  if (ba_sim3_robust_check(g->F, kind, scale)) return -1;
  return ba::graph_set_robust(g, kind, scale);
}

int ba_sim3_factor_weights(ba_sim3 *g, double *s, double *w) {
  if (!g) return fail("ba_sim3_factor_weights: null graph");
  return ba::graph_factor_weights(kS3Spec, g, s, w);
}

int ba_sim3_cov_check(int n_pose, const uint8_t *pose_fixed, int n_pose_sel, const int32_t *pose_sel,
                      const double *cov_pose49, int64_t n_pair, const int32_t *pair_j, const int32_t *pair_k,
                      const double *cov_rel49, int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k,
                      const double *Z13, const double *Omega49, const double *d2) {
  std::string err;
  if (ba::sim3_cov_validate_host(n_pose, pose_fixed, n_pose_sel, pose_sel, cov_pose49, n_pair, pair_j, pair_k,
                                 cov_rel49, n_cand, cand_j, cand_k, Z13, Omega49, d2, &err))
    return fail(err);
  return 0;
}

int ba_sim3_covariance(ba_sim3 *g, int n_pose_sel, const int32_t *pose_sel, double *cov_pose49, int64_t n_pair,
                       const int32_t *pair_j, const int32_t *pair_k, double *cov_cross49, double *cov_rel49,
                       int64_t *dropped_pivots) {
  if (!g) return fail("ba_sim3_covariance: null graph");
  if (ba_sim3_cov_check(g->n_pose, g->fixed.data(), n_pose_sel, pose_sel, cov_pose49, n_pair, pair_j, pair_k,
                        cov_rel49, 0, nullptr, nullptr, nullptr, nullptr, nullptr))
    return -1;
  return ba::graph_covariance(kS3Spec, g, n_pose_sel, pose_sel, cov_pose49, n_pair, pair_j, pair_k, cov_cross49,
                              cov_rel49, dropped_pivots);
}

int ba_sim3_gate(ba_sim3 *g, int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k, const double *Z13,
                 const double *Omega49, double *d2, double *r7, double *innov49, int64_t *dropped_pivots) {
  if (!g) return fail("ba_sim3_gate: null graph");
  if (ba_sim3_cov_check(g->n_pose, g->fixed.data(), 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, n_cand,
                        cand_j, cand_k, Z13, Omega49, d2))
    return -1;
  return ba::graph_gate(kS3Spec, g, n_cand, cand_j, cand_k, Z13, Omega49, d2, r7, innov49, dropped_pivots);
}

int ba_sim3_cov_info(ba_sim3 *g, int64_t out4[4]) {
  if (!g || !out4) return fail("ba_sim3_cov_info: bad argument");
  ba::graph_cov_info(g, out4);
  return 0;
}

int ba_sim3_solve(ba_sim3 *g, const ba_options *opt, ba_iter_info *rows, int cap, int *n_iter, int *converged) {
  if (!g || !opt) return fail("ba_sim3_solve: bad argument");
  if (cap < 0 || (cap > 0 && !rows)) return fail("ba_sim3_solve: rows is NULL for cap > 0");
  return ba::graph_solve(kS3Spec, g, opt, rows, cap, n_iter, converged);
}

int ba_sim3_get_poses(ba_sim3 *g, double *S13) {
  if (!g || !S13) return fail("ba_sim3_get_poses: bad argument");
  return ba::graph_get_poses(kS3Spec, g, S13);
}

int ba_sim3_cost(ba_sim3 *g, double *chi2) {
  if (!g || !chi2) return fail("ba_sim3_cost: bad argument");
  return ba::graph_cost(kS3Spec, g, chi2);
}

int ba_sim3_get_system(ba_sim3 *g, double *H, double *g7N) {
  if (!g) return fail("ba_sim3_get_system: null graph");
  return ba::graph_get_system(kS3Spec, g, H, g7N);
}

int ba_sim3_info(ba_sim3 *g, int64_t out9[9]) {
  if (!g || !out9) return fail("ba_sim3_info: bad argument");
  ba::graph_info(g, out9);
  out9[8] = ba::kS3Fpb;
  return 0;
}

int ba_sim3_last_ms(ba_sim3 *g, double *ms) {
  if (!g || !ms) return fail("ba_sim3_last_ms: bad argument");
  *ms = ba::graph_last_ms(g);
  return 0;
}

}  // extern "C"
