// ba_pgraph.hip — pose-graph optimisation (ba_pgraph_*, include/ba_hip.h):
// Levenberg-Marquardt over relative-pose factors alone, chi2 = sum_f r_f^T Omega_f r_f.  The
// reference project has no counterpart; the definition is the comment in include/ba_hip.h.
// The factor arithmetic is defined once, in ba_rel_fn.h, the linear solve is
// the level-scheduled tile Cholesky of ba_dense.hip.  Four kernels:
//   k_pg_lin       kPgFpb factors per workgroup: r and Ad per factor into LDS, then one thread
//                  per element of Omega Ad, Omega r, Ad^T Omega Ad, Ad^T Omega r; the 84-double
//                  record of a factor leaves in runs of 36 / 6 consecutive doubles (Ad and r
//                  never leave LDS); the workgroup's chi-square partial.  Cost-only mode: the
//                  partial alone
//   k_pg_assemble  one thread per element of H_jj / g_j walks the pose's list, one per element
//                  of a coupled block the block's list, in input order; H + lambda diag(H) and
//                  g go straight into the dense image, diag(H) and g are kept for pred
//   k_pg_trial     one thread per optimisable pose: T_j <- se3_exp(x_j) T_j into the other pose
//                  buffer; partials of sum |x_j| and of pred
//   k_pg_control   one workgroup: the sums, rho, status, lambda, the buffer swap, the stop test,
//                  the log row
// One writer per element, fixed trees, no floating-point atomics: the same bits run to run.
// Robust kernels (ba_pgraph_set_robust): k_pg_lin_robust and k_pg_assemble_robust
// are second instantiations of the two bodies with sum rho(s) for chi-square and w Omega for
// Omega; a graph whose kinds are all 0 launches the plain ones.
// The host side is the graph driver of ba_graph.hip, which this graph shares with the Sim(3) one
// (ba_sim3.hip): below the kernels this file has the driver's description of an SE(3) graph
// (kPgSpec: the widths, these launchers) and the ba_pgraph_* entry points, which validate and call
// the driver.  Covariance blocks and the gate (ba_pgraph_covariance / ba_pgraph_gate; DESIGN.md
// §6m): the driver's graph_cov_run (the solve's launches at lambda = 0, then column batches), the
// groups and the validation in ba_pgraph_host.h, the kernels in ba_pgraph_cov.hip.
#include <type_traits>

#include "ba_graph.h"
#include "ba_rel_fn.h"
#include "ba_robust_fn.h"

namespace ba {
namespace {

constexpr int kPgBlock = 256;
constexpr int kPgAdS = 37, kPgRS = 7;  // odd strides of the per-factor LDS rows: no bank conflicts
inline int pg_cdiv(int64_t a, int b) { return (int)((a + b - 1) / b); }

// (rho(s) and w = rho'(s) of one factor: pg_rho of ba_robust_fn.h, shared with ba_sim3.hip)

// The robust record as a kernel argument: an empty struct for the plain instantiation
struct PgNoRobust {};
template <bool kRobust>
using PgRobustArg = typename std::conditional<kRobust, PgRobust, PgNoRobust>::type;

// kRobust = false is the kernel of §6k: every robust line is compiled out
template <bool kRobust>
__global__ __launch_bounds__(kPgBlock) void k_pg_lin_t(PgDev p, int cost_only, PgRobustArg<kRobust> rb) {
  __shared__ double sAd[kPgFpb * kPgAdS], sOA[kPgFpb * kPgAdS], sR[kPgFpb * kPgRS], sOr[kPgFpb * kPgRS];
  __shared__ double sm[4];
  __shared__ double sW[kRobust ? kPgFpb : 1];
  const PgCtrl *c = p.ctrl;
  if (c->done) return;
  if (!cost_only && !c->relin) return;  // a rejected step: the records still belong to the accepted poses
  const double *P = p.poses[cost_only == 1 ? c->cur ^ 1 : c->cur];
  const int f0 = blockIdx.x * kPgFpb;
  const int nf = min(kPgFpb, p.F - f0);
  const int tid = threadIdx.x;
  const double *val = p.val + (size_t)f0 * 48;
  double q = 0.0;
  if (tid < nf) {
    const int4 jk = p.jk[f0 + tid];
    double RE[9], tE[3], rr[6];
    rel_E(jk, P, RE, tE);
    const double *Z = val + (size_t)tid * 48, *Om = Z + 12;
    rel_log(RE, tE, Z, rr);
    q = rel_quad(Om, rr);
    if constexpr (kRobust) {  // the partial is sum rho(s); w rides through LDS to the element threads
      double w;
      const double s = q;
      q = pg_rho(rb.kind[f0 + tid], rb.scale[f0 + tid], s, &w);
      if (!cost_only) sW[tid] = w;
      if (cost_only == 0 || cost_only == 3) {
        rb.s[f0 + tid] = s;
        rb.w[f0 + tid] = w;
      }
    }
    if (!cost_only) {  // r and Ad
      rel_Ad(RE, tE, sAd + tid * kPgAdS);
#pragma unroll
      for (int a = 0; a < 6; ++a) sR[tid * kPgRS + a] = rr[a];
    }
  }
  if (!cost_only) {
    double *rec = p.rec + (size_t)f0 * kPgRec;
    __syncthreads();
    // OA = Omega Ad and Or = Omega r, one thread per element
    for (int e = tid; e < 42 * nf; e += kPgBlock) {
      const int f = e / 42, k = e - 42 * f;
      const double *Om = val + (size_t)f * 48 + 12;
      if (k < 36) {
        double acc = rel_OA(Om, sAd + f * kPgAdS, k);
        if constexpr (kRobust) acc *= sW[f];
        sOA[f * kPgAdS + k] = acc;
        rec[(size_t)f * kPgRec + kPgOA + k] = acc;
      } else {
        const int a = k - 36;
        double acc = rel_Or(Om, sR + f * kPgRS, a);
        if constexpr (kRobust) acc *= sW[f];
        sOr[f * kPgRS + a] = acc;
        rec[(size_t)f * kPgRec + kPgOr + a] = acc;
      }
    }
    __syncthreads();
    // Bk = Ad^T OA and gk = Ad^T Or, for the factors whose k is optimisable
    for (int e = tid; e < 42 * nf; e += kPgBlock) {
      const int f = e / 42, k = e - 42 * f;
      if (p.jk[f0 + f].w < 0) continue;
      if (k < 36) {
        rec[(size_t)f * kPgRec + kPgBk + k] = rel_Bk(sAd + f * kPgAdS, sOA + f * kPgAdS, k);
      } else {
        const int a = k - 36;
        rec[(size_t)f * kPgRec + kPgGk + a] = rel_gk(sAd + f * kPgAdS, sOr + f * kPgRS, a);
      }
    }
  }
  const double tot = block_sum(q, sm);
  if (tid == 0) p.part[cost_only ? 1 : 0][blockIdx.x] = tot;
}

template <bool kRobust>
__global__ __launch_bounds__(kPgBlock) void k_pg_assemble_t(PgDev p, double *Hout, double *gout,
                                                            PgRobustArg<kRobust> rb) {
  const PgCtrl *c = p.ctrl;
  if (c->done) return;
  const int64_t e = (int64_t)blockIdx.x * kPgBlock + threadIdx.x;
  const int64_t nd = (int64_t)42 * p.N;
  const size_t n6 = (size_t)6 * p.N;
  if (e < nd) {
    const int j = (int)(e / 42), q = (int)(e - (int64_t)42 * j);
    // (the two walks are rel_walk_pose / rel_walk_block of ba_rel_fn.h written out: calling
    // them measured 2 % slower here, see profiles/rel_shared_v1.txt)
    const int l1 = p.pptr[j + 1];
    double acc = 0.0;
    for (int l = p.pptr[j]; l < l1; ++l) {
      const int w = p.plist[l], f = w >> 1;
      const double *rec = p.rec + (size_t)f * kPgRec;
      if (q < 36)
        if constexpr (kRobust)  // H_jj += w Omega: the one term that is not read from the records
          acc += (w & 1) ? rec[kPgBk + q] : rb.w[f] * p.val[(size_t)f * 48 + 12 + q];
        else
          acc += (w & 1) ? rec[kPgBk + q] : p.val[(size_t)f * 48 + 12 + q];
      else
        acc += (w & 1) ? rec[kPgGk + q - 36] : -rec[kPgOr + q - 36];
    }
    const int pc = p.pose_col[j];
    if (q < 36) {
      const int rw = q / 6, cc = q - 6 * rw;
      if (Hout) {
        Hout[((size_t)6 * j + rw) * n6 + (size_t)6 * j + cc] = acc;
      } else {
        if (rw == cc) {
          p.dH[6 * j + rw] = acc;
          acc = acc + c->lambda * acc;
        }
        if (rw >= cc) p.L[(size_t)(pc + cc) * p.ld + pc + rw] = acc;
      }
    } else {
      const int r = q - 36;
      if (Hout) {
        gout[6 * j + r] = acc;
      } else {
        p.g[6 * j + r] = acc;
        p.L[(size_t)(pc + r) * p.ld + p.npad] = acc;  // the right-hand side rides as row npad
      }
    }
    return;
  }
  const int64_t eb = e - nd;
  if (eb >= (int64_t)36 * p.nblk) return;
  const int b = (int)(eb / 36), rc = (int)(eb - (int64_t)36 * b), r = rc / 6, cc = rc - 6 * r;
  const int2 hl = p.blk[b];
  const int l1 = p.bptr[b + 1];
  double acc = 0.0;
  for (int l = p.bptr[b]; l < l1; ++l) {
    const int w = p.blist[l], f = w >> 1;
    acc -= p.rec[(size_t)f * kPgRec + kPgOA + ((w & 1) ? cc * 6 + r : rc)];
  }
  if (Hout) {
    Hout[((size_t)6 * hl.x + r) * n6 + (size_t)6 * hl.y + cc] = acc;
    Hout[((size_t)6 * hl.y + cc) * n6 + (size_t)6 * hl.x + r] = acc;
    return;
  }
  // element (r, cc) of H_hi,lo; where the column map puts it above the diagonal it is stored
  // transposed, so that the lower triangle of the image is complete
  const int row = p.pose_col[hl.x] + r, col = p.pose_col[hl.y] + cc;
  p.L[row > col ? (size_t)col * p.ld + row : (size_t)row * p.ld + col] = acc;
}

// the names the kernel table lists: k_pg_lin / k_pg_assemble and their robust instantiations
constexpr auto k_pg_lin = k_pg_lin_t<false>;
constexpr auto k_pg_lin_robust = k_pg_lin_t<true>;
constexpr auto k_pg_assemble = k_pg_assemble_t<false>;
constexpr auto k_pg_assemble_robust = k_pg_assemble_t<true>;

__global__ __launch_bounds__(kPgBlock) void k_pg_trial(PgDev p) {
  __shared__ double sm[8];
  const PgCtrl *c = p.ctrl;
  if (c->done) return;
  const int j = blockIdx.x * kPgBlock + threadIdx.x;
  double sx = 0.0, pr = 0.0;
  if (j < p.N) {
    const double *xj = p.x + (size_t)6 * j;
    const double v0 = xj[0], v1 = xj[1], v2 = xj[2], w0 = xj[3], w1 = xj[4], w2 = xj[5];
    double dR[9], dt[3];
    se3_exp(v0, v1, v2, w0, w1, w2, dR, dt);
    const int ps = p.opt_pose[j];
    const double *T = p.poses[c->cur] + (size_t)ps * 12;
    double *To = p.poses[c->cur ^ 1] + (size_t)ps * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int cc = 0; cc < 3; ++cc)
        To[r * 3 + cc] = dR[r * 3 + 0] * T[0 * 3 + cc] + dR[r * 3 + 1] * T[1 * 3 + cc] + dR[r * 3 + 2] * T[2 * 3 + cc];
      To[9 + r] = dR[r * 3 + 0] * T[9] + dR[r * 3 + 1] * T[10] + dR[r * 3 + 2] * T[11] + dt[r];
    }
    double gx = 0.0, dx = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      gx += p.g[6 * j + r] * xj[r];
      dx += (xj[r] * p.dH[6 * j + r]) * xj[r];
    }
    pr = gx + c->lambda * dx;  // pred = g^T x + lambda x^T diag(H) x
    sx = sqrt(v0 * v0 + v1 * v1 + v2 * v2 + w0 * w0 + w1 * w1 + w2 * w2);
  }
  block_sum2(sx, pr, sm);
  if (threadIdx.x == 0) {
    p.tpart[2 * blockIdx.x + 0] = sx;
    p.tpart[2 * blockIdx.x + 1] = pr;
  }
}

__global__ __launch_bounds__(kPgBlock) void k_pg_control(PgDev p, int mode) {
  __shared__ double sm[8];
  PgCtrl *c = p.ctrl;
  if (c->done) return;
  double a = 0.0, t = 0.0, sx = 0.0, pr = 0.0;
  for (int k = threadIdx.x; k < p.n_part; k += kPgBlock) {
    a += p.part[0][k];
    t += p.part[1][k];
  }
  block_sum2(a, t, sm);
  if (mode == 1) {
    if (threadIdx.x == 0) c->aux = t;
    return;
  }
  for (int k = threadIdx.x; k < p.n_tpart; k += kPgBlock) {
    sx += p.tpart[2 * k + 0];
    pr += p.tpart[2 * k + 1];
  }
  block_sum2(sx, pr, sm);
  if (threadIdx.x != 0) return;
  if (c->iter == 0) c->chi2 = a;  // the chi-square of the start: the first linearisation's
  const double accepted = c->chi2, trial = t;
  double lambda = c->lambda, rho, pred;
  int status;
  bool accept;
  if (c->gn) {
    status = 0;
    rho = 0.0;
    pred = 0.0;
    accept = true;
  } else {
    pred = pr;
    rho = (accepted - trial) / pred;
    accept = rho > 0.25;
    status = accept ? 0 : 2;
    if (rho > 0.5) {
      lambda = fmax(1e-10, lambda * c->dec_ratio);
      status = 1;
    } else if (!accept) {
      lambda = fmin(1e10, lambda * c->inc_ratio);
    }
  }
  const double change = fabs(accepted - trial);
  const double mean_step = sx / (double)p.N;
  bool conv = (mean_step < c->thr_step) || (change < c->thr_cost);
  if (c->iter >= c->max_iter - 1) conv = false;
  const double cost = accept ? trial : accepted;
  const unsigned long long now = wall_clock64();
  if (c->iter < p.log_cap) {
    DevIterRec &I = p.log[c->iter];
    I.cost = cost;
    I.cost_change = accept ? change : 0.0;
    I.average_reprojection_error = sqrt(cost / (double)p.F);
    I.abs_gradient = 0.0;
    I.abs_step = mean_step;
    I.damping_term = lambda;
    I.iter_time_ms = (double)(now - c->t_last) * 1e-5;  // 100 MHz clock
    I.iteration_status = status;
    I.pad_ = 0;
    I.rho = rho;
    I.model_change = pred;
    I.trial_cost = trial;
  }
  c->t_last = now;
  c->lambda = lambda;
  c->chi2 = cost;  // a rejected step leaves the accepted chi-square the comparison value
  if (accept) c->cur ^= 1;
  c->relin = accept ? 1 : 0;
  c->iter += 1;
  c->converged = conv ? 1 : 0;
  if (conv || c->iter >= c->max_iter) c->done = 1;
}

}  // namespace

void launch_pg_lin(const PgDev &p, int cost_only, hipStream_t s) {
  BA_LAUNCH(K_PG_LIN, k_pg_lin, dim3(p.n_part), dim3(kPgBlock), s, p, cost_only, PgNoRobust{});
}
void launch_pg_assemble(const PgDev &p, double *Hout, double *gout, hipStream_t s) {
  const int grid = pg_cdiv((int64_t)42 * p.N + (int64_t)36 * p.nblk, kPgBlock);
  BA_LAUNCH(K_PG_ASSEMBLE, k_pg_assemble, dim3(grid), dim3(kPgBlock), s, p, Hout, gout, PgNoRobust{});
}
void launch_pg_lin_robust(const PgDev &p, const PgRobust &rb, int cost_only, hipStream_t s) {
  BA_LAUNCH(K_PG_LIN_ROBUST, k_pg_lin_robust, dim3(p.n_part), dim3(kPgBlock), s, p, cost_only, rb);
}
void launch_pg_assemble_robust(const PgDev &p, const PgRobust &rb, double *Hout, double *gout, hipStream_t s) {
  const int grid = pg_cdiv((int64_t)42 * p.N + (int64_t)36 * p.nblk, kPgBlock);
  BA_LAUNCH(K_PG_ASSEMBLE_ROBUST, k_pg_assemble_robust, dim3(grid), dim3(kPgBlock), s, p, Hout, gout, rb);
}
void launch_pg_trial(const PgDev &p, hipStream_t s) {
  BA_LAUNCH(K_PG_TRIAL, k_pg_trial, dim3(p.n_tpart), dim3(kPgBlock), s, p);
}
void launch_pg_control(const PgDev &p, int mode, hipStream_t s) {
  BA_LAUNCH(K_PG_CONTROL, k_pg_control, dim3(1), dim3(kPgBlock), s, p, mode);
}

}  // namespace ba

// ---- host side ------------------------------------------------------------------------------
// The driver is ba_graph.hip; here are the SE(3) graph's spec and its entry points, which check
// their pointers, validate the caller's arrays and call the driver.
using ba::fail;

struct ba_pgraph : ba::GraphHost {};

namespace {

void pg_cov_batch(const ba::PgDev &p, const double *Ldiag, int nb, int ncb, const double *poses, const int *trow_ptr,
                  const int *trow, const ba::PgCovGroup *groups, int ng, const double *cand_val, double *Zw, int bw,
                  const ba::GraphCovOut &o, hipStream_t s) {
  const ba::PgCovOut out{o.pose, o.cross, o.rel, o.r, o.innov, o.d2};
  ba::launch_pgcov_batch(p, Ldiag, nb, ncb, poses, trow_ptr, trow, groups, ng, cand_val, Zw, bw, out, s);
}

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
    ba::launch_pg_lin,
    ba::launch_pg_lin_robust,
    ba::launch_pg_assemble,
    ba::launch_pg_assemble_robust,
    ba::launch_pg_trial,
    pg_cov_batch,
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
