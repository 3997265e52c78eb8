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
// Covariance blocks and the gate (ba_pgraph_covariance / ba_pgraph_gate): the host
// side is here (pg_cov_run: the solve's launches at lambda = 0, then column batches), the groups
// and the validation in ba_pgraph_host.h, the kernels in ba_pgraph_cov.hip.
#include <cstddef>
#include <cstring>
#include <type_traits>

#include "ba_handle.h"
#include "ba_pgraph_host.h"
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
using ba::fail;
using ba::Mem;

struct ba_pgraph {
  ba_handle *h = nullptr;
  int n_pose = 0;
  int64_t F = 0;
  std::vector<uint8_t> fixed;
  std::vector<int32_t> rel_j, rel_k;
  std::vector<double> Z, Om;  // the factor values as given (ba_pgraph_update_values replaces one or both)
  ba::PgraphLists lists;
  ba::DenseSchedule sched;
  ba::DenseDev dd;
  ba::PgDev d{};
  ba::PgCtrl hc{};
  double *Ldiag = nullptr, *val = nullptr;
  // robust kernels: the host copy as given, the device arrays (allocated by the first
  // ba_pgraph_set_robust or ba_pgraph_factor_report), and whether any kind is not 0
  std::vector<int32_t> rkind;
  std::vector<double> rscale;
  int32_t *d_rkind = nullptr;
  double *d_rscale = nullptr, *d_rep_s = nullptr, *d_rep_w = nullptr;
  ba::PgRobust rb{};
  bool robust = false;
  int *zt_I = nullptr, *zt_J = nullptr, *col_x = nullptr;
  int n_zt = 0, nb = 0, ncb = 0;
  size_t image_bytes = 0;
  int64_t bad_pivots = 0;
  double last_ms = 0.0;
  std::vector<int> pose_col_h;  // per optimisable pose: its first column of the image
  int cov_batches = 0;          // column batches of the last ba_pgraph_covariance / ba_pgraph_gate
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<void *> allocs;
};

namespace {

// what was allocated on the handle since `mark` belongs to the graph from here on
void adopt_allocs(ba_pgraph *g, size_t mark) {
  ba_handle *h = g->h;
  g->allocs.insert(g->allocs.end(), h->allocs.begin() + mark, h->allocs.end());
  h->allocs.resize(mark);
}

void free_graph(ba_pgraph *g) {
  for (void *p : g->allocs) (void)hipFree(p);
  if (g->e0) (void)hipEventDestroy(g->e0);
  if (g->e1) (void)hipEventDestroy(g->e1);
  delete g;
}

int push_ctrl(ba_pgraph *g) {
  HIP_TRY(hipMemcpyAsync(g->d.ctrl, &g->hc, sizeof(ba::PgCtrl), hipMemcpyHostToDevice, g->h->stream));
  return 0;
}
int pull_ctrl(ba_pgraph *g) {
  HIP_TRY(hipMemcpyAsync(&g->hc, g->d.ctrl, sizeof(ba::PgCtrl), hipMemcpyDeviceToHost, g->h->stream));
  HIP_TRY(hipStreamSynchronize(g->h->stream));
  return 0;
}
const int *done_flag(const ba_pgraph *g) {
  return (const int *)((const char *)g->d.ctrl + offsetof(ba::PgCtrl, done));
}

// the device side of a validated graph; on failure the caller frees what `g` holds
int build_device(ba_pgraph *g, const double *T_jw12) {
  ba_handle *h = g->h;
  const ba::PgraphLists &l = g->lists;
  const ba::DenseKnobs &knobs = h->knobs.dense;
  ba::PgDev &d = g->d;
  const int N = l.N;
  // both tile orders, as ba_finalize builds them for the reduced camera system
  ba::DenseSchedule cand[2];
  const int orders[2] = {32, 64};
  for (int k = 0; k < 2; ++k) {
    int ncb_k = 0;
    std::vector<uint8_t> adj;
    ba::pgraph_tile_adjacency(l, ba::dense_poses_per_tile(orders[k]), &ncb_k, &adj);
    if (knobs.full) std::fill(adj.begin(), adj.end(), 1);
    ba::build_dense_schedule(ncb_k, adj, knobs.natural, orders[k], cand[k], knobs.order);
  }
  g->sched = cand[ba::dense_pick_tile_order(cand[0], cand[1], knobs.nb)];
  const ba::DenseSchedule &sc = g->sched;
  const int nb = sc.nb, ppt = ba::dense_poses_per_tile(nb), ncb = sc.ncb;
  g->nb = nb;
  g->ncb = ncb;
  d.n_pose = g->n_pose;
  d.N = N;
  d.F = (int)g->F;
  d.nblk = (int)(l.blk.size() / 2);
  d.n_part = (int)((g->F + ba::kPgFpb - 1) / ba::kPgFpb);
  d.n_tpart = (N + 255) / 256;
  d.npad = ncb * nb;
  d.ld = d.npad + nb;
  d.log_cap = 4096;
  // the image first: nothing is launched, and nothing else allocated, if it does not fit
  g->image_bytes = (size_t)d.npad * d.ld * sizeof(double);
  {
    hipError_t e = hipMalloc((void **)&d.L, g->image_bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      d.L = nullptr;
      return fail("ba_pgraph_create: cannot allocate the dense image of " + std::to_string(d.npad) + " x " +
                  std::to_string(d.ld) + " doubles (" + std::to_string(g->image_bytes) + " bytes): " +
                  hipGetErrorString(e));
    }
    g->allocs.push_back((void *)d.L);
  }
  std::vector<int> pose_col((size_t)N, 0), col_x((size_t)d.npad, -1);
  for (int j = 0; j < N; ++j) {
    const int c0 = sc.pos_of_tile[j / ppt] * nb + 6 * (j % ppt);
    pose_col[j] = c0;
    for (int r = 0; r < 6; ++r) col_x[c0 + r] = 6 * j + r;
  }
  // tiles (re)initialised per iteration: factor pattern + diagonal + rhs row
  std::vector<int> ztI, ztJ;
  for (int p = 0; p < ncb; ++p) {
    ztI.push_back(p);
    ztJ.push_back(p);
    for (int q = sc.row_ptr[p]; q < sc.row_ptr[p + 1]; ++q) {
      ztI.push_back(sc.rows[q]);  // includes the rhs row block (== ncb)
      ztJ.push_back(p);
    }
  }
  g->n_zt = (int)ztI.size();
  g->pose_col_h = pose_col;
  std::vector<double> val;
  ba::relative_pack_values(g->F, g->Z.data(), g->Om.data(), &val);
  constexpr Mem R = Mem::Resident;
  static_assert(sizeof(int4) == 16 && sizeof(int2) == 8, "layout");
  int4 *jk = nullptr;
  int2 *blk = nullptr;
  int32_t *pptr = nullptr, *plist = nullptr, *bptr = nullptr, *blist = nullptr, *opt_pose = nullptr;
  int *pc = nullptr;
  const size_t n6 = (size_t)6 * N;
  if (ba::upload_dense_schedule(h, sc, col_x, g->dd) ||
      h->dalloc(R, &g->Ldiag, (size_t)ncb * ba::dense_ws_per_block(nb)) || h->upload(R, &pc, pose_col) ||
      h->upload(R, &g->zt_I, ztI) || h->upload(R, &g->zt_J, ztJ) ||
      h->upload(R, &d.poses[0], T_jw12, (size_t)g->n_pose * 12) ||
      h->upload(R, &d.poses[1], T_jw12, (size_t)g->n_pose * 12) || h->upload(R, &jk, l.jk.data(), (size_t)g->F) ||
      h->upload(R, &g->val, val) || h->upload(R, &pptr, l.pptr) || h->upload(R, &plist, l.plist) ||
      h->upload(R, &blk, l.blk.data(), l.blk.size() / 2) || h->upload(R, &bptr, l.bptr) ||
      h->upload(R, &blist, l.blist) || h->upload(R, &opt_pose, l.opt_pose) ||
      h->dalloc(R, &d.rec, (size_t)g->F * ba::kPgRec) || h->dalloc(R, &d.dH, n6) || h->dalloc(R, &d.g, n6) ||
      h->dalloc(R, &d.x, n6 + 64) || h->dalloc(R, &d.part[0], (size_t)d.n_part) ||
      h->dalloc(R, &d.part[1], (size_t)d.n_part) || h->dalloc(R, &d.tpart, (size_t)2 * d.n_tpart) ||
      h->dalloc(R, &d.ctrl, (size_t)1) || h->dalloc(R, &d.log, (size_t)d.log_cap))
    return -1;
  g->col_x = g->dd.col_x;
  d.jk = jk;
  d.val = g->val;
  d.pptr = pptr;
  d.plist = plist;
  d.blk = blk;
  d.bptr = bptr;
  d.blist = blist;
  d.opt_pose = opt_pose;
  d.pose_col = pc;
  HIP_TRY(hipMemset(d.L, 0, g->image_bytes));
  HIP_TRY(hipMemset(d.rec, 0, (size_t)g->F * ba::kPgRec * sizeof(double)));
  HIP_TRY(hipMemset(d.dH, 0, n6 * sizeof(double)));
  HIP_TRY(hipMemset(d.g, 0, n6 * sizeof(double)));
  HIP_TRY(hipMemset(d.x, 0, (n6 + 64) * sizeof(double)));
  HIP_TRY(hipMemset(d.part[0], 0, (size_t)d.n_part * sizeof(double)));
  HIP_TRY(hipMemset(d.part[1], 0, (size_t)d.n_part * sizeof(double)));
  HIP_TRY(hipMemset(d.tpart, 0, (size_t)2 * d.n_tpart * sizeof(double)));
  HIP_TRY(hipMemset(d.ctrl, 0, sizeof(ba::PgCtrl)));
  HIP_TRY(hipEventCreate(&g->e0));
  HIP_TRY(hipEventCreate(&g->e1));
  return 0;
}

// the controller for a pass outside the LM loop: the accepted buffer stays
int begin_pass(ba_pgraph *g) {
  g->hc.done = 0;
  g->hc.relin = 1;
  g->hc.lambda = 0.0;
  return push_ctrl(g);
}

// the device arrays of the robust kernels: kinds 0 and the weights' arrays, once per graph
int ensure_robust_arrays(ba_pgraph *g) {
  if (g->d_rkind) return 0;
  ba_handle *h = g->h;
  constexpr Mem R = Mem::Resident;
  const size_t F = (size_t)g->F, mark = h->allocs.size();
  const int rc = h->dalloc(R, &g->d_rkind, F) || h->dalloc(R, &g->d_rscale, F) || h->dalloc(R, &g->rb.s, F) ||
                 h->dalloc(R, &g->rb.w, F) || h->dalloc(R, &g->d_rep_s, F) || h->dalloc(R, &g->d_rep_w, F);
  adopt_allocs(g, mark);
  if (rc) {
    g->d_rkind = nullptr;  // what was allocated goes with the graph
    return -1;
  }
  g->rb.kind = g->d_rkind;
  g->rb.scale = g->d_rscale;
  HIP_TRY(hipMemset(g->d_rkind, 0, F * sizeof(int32_t)));
  HIP_TRY(hipMemset(g->d_rscale, 0, F * sizeof(double)));
  return 0;
}

// the linearisation / cost pass and the assembly of the graph: the robust instantiations only
// where a kernel is set
void pg_lin(const ba_pgraph *g, int cost_only, hipStream_t s) {
  if (g->robust)
    ba::launch_pg_lin_robust(g->d, g->rb, cost_only, s);
  else
    ba::launch_pg_lin(g->d, cost_only, s);
}
void pg_assemble(const ba_pgraph *g, double *Hout, double *gout, hipStream_t s) {
  if (g->robust)
    ba::launch_pg_assemble_robust(g->d, g->rb, Hout, gout, s);
  else
    ba::launch_pg_assemble(g->d, Hout, gout, s);
}


template <class T>
int download(std::vector<T> &out, const T *dev, size_t n, hipStream_t s) {
  out.resize(n);
  if (n) HIP_TRY(hipMemcpyAsync(out.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
  return 0;
}

// The host arrays of one covariance or gate call (validated): entry_kind = kPgCovPair with
// Z12 = Omega36 = nullptr, or kPgCovCand.  Outputs that are null are not produced.
struct PgCovCall {
  int n_pose_sel = 0;
  const int32_t *pose_sel = nullptr;
  double *cov_pose36 = nullptr;
  int64_t n_entry = 0;
  int entry_kind = ba::kPgCovPair;
  const int32_t *entry_j = nullptr, *entry_k = nullptr;
  const double *Z12 = nullptr, *Omega36 = nullptr;
  double *cov_cross36 = nullptr, *cov_rel36 = nullptr, *d2 = nullptr, *r6 = nullptr, *innov36 = nullptr;
};

// Factorise H at lambda = 0 at the accepted poses with the solve's launches, sweep the groups
// in column batches, copy the blocks out.  The controller, the solve's count of dropped pivots
// and last_ms are as before on return; the workspace and the lists are freed on every path.
int pg_cov_run(ba_pgraph *g, const char *what, const PgCovCall &c, int64_t *dropped_pivots) {
  ba_handle *h = g->h;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const ba::PgDev &d = g->d;
  const ba::DenseSchedule &sc = g->sched;
  std::vector<ba::PgCovGroup> groups;
  std::vector<int32_t> slot_of_opt;
  int n_pose_rows = 0;
  ba::pgraph_cov_groups(g->lists, g->pose_col_h, g->nb, c.n_pose_sel, c.pose_sel, c.n_entry, c.entry_j, c.entry_k,
                        c.entry_kind, &groups, &slot_of_opt, &n_pose_rows);
  std::vector<int> trow_ptr, trow;
  ba::pgraph_cov_tile_rows(g->ncb, sc.row_ptr, sc.rows, &trow_ptr, &trow);
  // ---- the factor of H at lambda = 0, whole in the image (no level goes to k_chol_tail)
  HIP_TRY(hipStreamSynchronize(s));
  const ba::PgCtrl keep = g->hc;
  int bad_keep = 0, bad_now = 0;
  HIP_TRY(hipMemcpy(&bad_keep, g->dd.bad_pivots, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemsetAsync(g->dd.bad_pivots, 0, sizeof(int), s));
  if (begin_pass(g)) return -1;
  const int *done = done_flag(g);
  pg_lin(g, 0, s);
  ba::launch_dense_init(d.L, d.ld, g->col_x, g->zt_I, g->zt_J, g->n_zt, g->nb, done, s);
  pg_assemble(g, nullptr, nullptr, s);
  ba::dense_factor_solve(d.L, d.npad, d.ld, g->Ldiag, d.x, done, sc, g->dd,
                         ba::dense_launch_plan_no_tail(sc, h->knobs.dense, g->dd.flow_ok, g->dd.plan[1],
                                                       h->knobs.cone.want),
                         s);
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(&bad_now, g->dd.bad_pivots, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(g->dd.bad_pivots, &bad_keep, sizeof(int), hipMemcpyHostToDevice));
  g->hc = keep;  // the controller as it was
  if (push_ctrl(g)) return -1;
  HIP_TRY(hipStreamSynchronize(s));
  if (bad_now >= ba::kFlowTimeout) return fail(std::string(what) + ": a dataflow hand-off of the factorisation timed out");
  // ---- the batches; everything below is freed again on every return
  ba::ScratchAllocs scratch(h);
  constexpr Mem R = Mem::Resident;
  const bool cand = c.entry_kind == ba::kPgCovCand;
  const size_t ne = (size_t)c.n_entry;
  const int gpb = ba::cov_batch_cols(d.npad, h->knobs.run) / ba::kCovGroupCols;  // groups per batch
  const int bw = (int)std::min<size_t>(gpb, std::max<size_t>(1, groups.size())) * ba::kCovGroupCols;
  int *d_trow_ptr = nullptr, *d_trow = nullptr;
  ba::PgCovGroup *d_groups = nullptr;
  double *Zw = nullptr, *d_val = nullptr;
  ba::PgCovOut out{};
  g->cov_batches = 0;
  if (!groups.empty()) {
    std::vector<double> val;
    if (cand) ba::relative_pack_values(c.n_entry, c.Z12, c.Omega36, &val);
    if (h->upload(R, &d_trow_ptr, trow_ptr) || h->upload(R, &d_trow, trow) || h->upload(R, &d_groups, groups) ||
        h->dalloc(R, &Zw, (size_t)d.npad * bw) || h->dalloc(R, &out.pose36, (size_t)n_pose_rows * 36) ||
        h->dalloc(R, &out.rel36, ne * 36) || (c.cov_cross36 && h->dalloc(R, &out.cross36, ne * 36)) ||
        (cand && (h->upload(R, &d_val, val) || h->dalloc(R, &out.d2, ne))) ||
        (cand && c.r6 && h->dalloc(R, &out.r6, ne * 6)) || (cand && c.innov36 && h->dalloc(R, &out.innov36, ne * 36)))
      return -1;
    for (size_t g0 = 0; g0 < groups.size(); g0 += gpb) {  // fixed batch order
      const int ng = (int)std::min<size_t>(gpb, groups.size() - g0);
      ba::launch_pgcov_batch(d, g->Ldiag, g->nb, g->ncb, d.poses[keep.cur], d_trow_ptr, d_trow, d_groups + g0, ng, d_val,
                             Zw, bw, out, s);
      ++g->cov_batches;
    }
  }
  std::vector<double> hp, hrel, hcross, hd2, hr, hP;
  if (download(hp, out.pose36, (size_t)n_pose_rows * 36, s) || download(hrel, out.rel36, out.rel36 ? ne * 36 : 0, s) ||
      download(hcross, out.cross36, out.cross36 ? ne * 36 : 0, s) || download(hd2, out.d2, out.d2 ? ne : 0, s) ||
      download(hr, out.r6, out.r6 ? ne * 6 : 0, s) || download(hP, out.innov36, out.innov36 ? ne * 36 : 0, s))
    return -1;
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  for (int q = 0; q < c.n_pose_sel; ++q)
    std::memcpy(c.cov_pose36 + (size_t)q * 36, &hp[(size_t)slot_of_opt[g->lists.opt_of_pose[c.pose_sel[q]]] * 36],
                36 * sizeof(double));
  auto give = [](double *dst, const std::vector<double> &src) {
    if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(double));
  };
  if (!cand) give(c.cov_rel36, hrel);
  give(c.cov_cross36, hcross);
  give(c.d2, hd2);
  give(c.r6, hr);
  give(c.innov36, hP);
  if (dropped_pivots) *dropped_pivots = bad_now;
  return 0;
}

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
  HIP_TRY(hipSetDevice(h->device));
  ba_pgraph *g = new ba_pgraph();
  g->h = h;
  g->n_pose = n_pose;
  g->F = n_rel;
  if (pose_fixed)
    g->fixed.assign(pose_fixed, pose_fixed + n_pose);
  else
    g->fixed.assign((size_t)n_pose, 0);
  g->rel_j.assign(rel_j, rel_j + n_rel);
  g->rel_k.assign(rel_k, rel_k + n_rel);
  g->Z.assign(Z12, Z12 + 12 * (size_t)n_rel);
  g->Om.assign(Omega36, Omega36 + 36 * (size_t)n_rel);
  ba::pgraph_build_lists(n_pose, g->fixed.data(), n_rel, rel_j, rel_k, &g->lists);
  const size_t mark = h->allocs.size();
  const int rc = build_device(g, T_jw12);
  adopt_allocs(g, mark);
  if (rc) {
    free_graph(g);
    return -1;
  }
  *out = g;
  return 0;
}

void ba_pgraph_destroy(ba_pgraph *g) {
  if (!g) return;
  (void)hipSetDevice(g->h->device);
  (void)hipStreamSynchronize(g->h->stream);
  free_graph(g);
}

int ba_pgraph_update_values(ba_pgraph *g, const double *T_jw12, const double *Z12, const double *Omega36) {
  if (!g) return fail("ba_pgraph_update_values: null graph");
  ba_handle *h = g->h;
  std::string err;
  if (T_jw12)
    for (int64_t e = 0; e < (int64_t)g->n_pose * 12; ++e)
      if (!std::isfinite(T_jw12[e]))
        return fail("ba_pgraph_update_values: T_jw is not finite (pose " + std::to_string(e / 12) + ")");
  if (Z12 || Omega36) {
    const double *Zn = Z12 ? Z12 : g->Z.data(), *On = Omega36 ? Omega36 : g->Om.data();
    if (ba::relative_validate_host(ba::kRelValues, g->n_pose, g->fixed.data(), g->F, nullptr, nullptr, Zn, On, &err))
      return fail("ba_pgraph_update_values: " + err);
  }
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (Z12 || Omega36) {
    if (Z12) g->Z.assign(Z12, Z12 + 12 * (size_t)g->F);
    if (Omega36) g->Om.assign(Omega36, Omega36 + 36 * (size_t)g->F);
    std::vector<double> val;
    ba::relative_pack_values(g->F, g->Z.data(), g->Om.data(), &val);
    HIP_TRY(hipMemcpy(g->val, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (T_jw12) {
    const size_t bytes = (size_t)g->n_pose * 12 * sizeof(double);
    HIP_TRY(hipMemcpy(g->d.poses[0], T_jw12, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g->d.poses[1], T_jw12, bytes, hipMemcpyHostToDevice));
    g->hc.cur = 0;
  }
  return 0;
}

int ba_pgraph_robust_check(int64_t n_rel, const int32_t *kind, const double *scale) {
  std::string err;
  if (ba::pgraph_robust_validate_host(n_rel, kind, scale, &err)) return fail("ba_pgraph_set_robust: " + err);
  return 0;
}

int ba_pgraph_set_robust(ba_pgraph *g, const int32_t *kind, const double *scale) {
  if (!g) return fail("ba_pgraph_set_robust: null graph");
  if (ba_pgraph_robust_check(g->F, kind, scale)) return -1;
  const size_t F = (size_t)g->F;
  std::vector<int32_t> k(F, 0);
  std::vector<double> c(F, 0.0);
  bool any = false;
  for (size_t f = 0; kind && f < F; ++f)
    if (kind[f] != 0) {
      k[f] = kind[f];
      c[f] = scale[f];
      any = true;
    }
  if (!any && !g->d_rkind) {  // never robust, and stays so: nothing to allocate
    g->robust = false;
    return 0;
  }
  ba_handle *h = g->h;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (ensure_robust_arrays(g)) return -1;
  HIP_TRY(hipMemcpy(g->d_rkind, k.data(), F * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(g->d_rscale, c.data(), F * sizeof(double), hipMemcpyHostToDevice));
  g->rkind.swap(k);
  g->rscale.swap(c);
  g->robust = any;
  return 0;
}

int ba_pgraph_factor_report(ba_pgraph *g, double *s, double *w) {
  if (!g) return fail("ba_pgraph_factor_report: null graph");
  ba_handle *h = g->h;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (ensure_robust_arrays(g)) return -1;
  if (begin_pass(g)) return -1;
  // one cost-only pass at the accepted poses; the report has arrays of its own, so that rb.s and
  // rb.w stay those of the records
  ba::PgRobust rep = g->rb;
  rep.s = g->d_rep_s;
  rep.w = g->d_rep_w;
  ba::launch_pg_lin_robust(g->d, rep, 3, h->stream);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  const size_t bytes = (size_t)g->F * sizeof(double);
  if (s) HIP_TRY(hipMemcpy(s, g->d_rep_s, bytes, hipMemcpyDeviceToHost));
  if (w) HIP_TRY(hipMemcpy(w, g->d_rep_w, bytes, hipMemcpyDeviceToHost));
  return 0;
}

int ba_pgraph_solve(ba_pgraph *g, const ba_options *opt,ba_iter_info *rows, int cap, int *n_iter, int *converged) {
  if (!g || !opt) return fail("ba_pgraph_solve: bad argument");
  if (cap < 0 || (cap > 0 && !rows)) return fail("ba_pgraph_solve: rows is NULL for cap > 0");
  ba_handle *h = g->h;
  if (n_iter) *n_iter = 0;
  if (converged) *converged = 1;
  if (opt->max_num_iterations <= 0) return 0;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const ba::PgDev &d = g->d;
  ba::PgCtrl &c = g->hc;
  const int cur = c.cur;
  std::memset(&c, 0, sizeof(c));
  c.cur = cur;
  c.lambda = (double)opt->initial_lambda;
  c.thr_step = (double)opt->threshold_step_size;
  c.thr_cost = (double)opt->threshold_cost_change;
  c.dec_ratio = (double)opt->decrease_ratio_lambda;
  c.inc_ratio = (double)opt->increase_ratio_lambda;
  c.max_iter = opt->max_num_iterations;
  c.gn = opt->gauss_newton ? 1 : 0;
  c.relin = 1;
  if (push_ctrl(g)) return -1;
  HIP_TRY(hipMemsetAsync(g->dd.bad_pivots, 0, sizeof(int), s));
  ba::g_ktimer = h->timing ? &h->kt : nullptr;
  const int *done = done_flag(g);
  HIP_TRY(hipEventRecord(g->e0, s));
  for (int it = 0; it < opt->max_num_iterations; ++it) {
    pg_lin(g, 0, s);
    ba::launch_dense_init(d.L, d.ld, g->col_x, g->zt_I, g->zt_J, g->n_zt, g->nb, done, s);
    pg_assemble(g, nullptr, nullptr, s);
    ba::dense_factor_solve(d.L, d.npad, d.ld, g->Ldiag, d.x, done, g->sched, g->dd, g->dd.plan[g->dd.flow_ok], s);
    ba::launch_pg_trial(d, s);
    pg_lin(g, 1, s);
    ba::launch_pg_control(d, 0, s);
  }
  HIP_TRY(hipEventRecord(g->e1, s));
  ba::g_ktimer = nullptr;
  if (pull_ctrl(g)) return -1;
  if (h->timing) h->kt.collect();
  HIP_TRY(hipGetLastError());
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, g->e0, g->e1);
  g->last_ms = ms;
  int bad = 0;
  HIP_TRY(hipMemcpy(&bad, g->dd.bad_pivots, sizeof(int), hipMemcpyDeviceToHost));
  if (bad >= ba::kFlowTimeout) return fail("ba_pgraph_solve: a dataflow hand-off timed out");
  g->bad_pivots = bad;
  static_assert(sizeof(ba::DevIterRec) == sizeof(ba_iter_info), "row layout");
  const int n = std::min(std::min(c.iter, cap), d.log_cap);
  if (n > 0) HIP_TRY(hipMemcpy(rows, d.log, (size_t)n * sizeof(ba_iter_info), hipMemcpyDeviceToHost));
  if (n_iter) *n_iter = c.iter;
  if (converged) *converged = c.converged;
  return 0;
}

int ba_pgraph_get_poses(ba_pgraph *g, double *T_jw12) {
  if (!g || !T_jw12) return fail("ba_pgraph_get_poses: bad argument");
  HIP_TRY(hipSetDevice(g->h->device));
  HIP_TRY(hipStreamSynchronize(g->h->stream));
  HIP_TRY(hipMemcpy(T_jw12, g->d.poses[g->hc.cur], (size_t)g->n_pose * 12 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int ba_pgraph_cost(ba_pgraph *g, double *chi2) {
  if (!g || !chi2) return fail("ba_pgraph_cost: bad argument");
  HIP_TRY(hipSetDevice(g->h->device));
  if (begin_pass(g)) return -1;
  pg_lin(g, 2, g->h->stream);
  ba::launch_pg_control(g->d, 1, g->h->stream);
  if (pull_ctrl(g)) return -1;
  HIP_TRY(hipGetLastError());
  *chi2 = g->hc.aux;
  return 0;
}

int ba_pgraph_get_system(ba_pgraph *g, double *H, double *g6N) {
  if (!g) return fail("ba_pgraph_get_system: null graph");
  ba_handle *h = g->h;
  HIP_TRY(hipSetDevice(h->device));
  const size_t n6 = (size_t)6 * g->d.N;
  double *dH = nullptr, *dg = nullptr;
  HIP_TRY(hipMalloc((void **)&dH, n6 * n6 * sizeof(double)));
  if (hipMalloc((void **)&dg, n6 * sizeof(double)) != hipSuccess) {
    (void)hipFree(dH);
    return fail("ba_pgraph_get_system: hipMalloc");
  }
  int rc = 0;
  if (hipMemsetAsync(dH, 0, n6 * n6 * sizeof(double), h->stream) != hipSuccess || begin_pass(g)) rc = -1;
  if (!rc) {
    pg_lin(g, 0, h->stream);
    pg_assemble(g, dH, dg, h->stream);
    if (hipStreamSynchronize(h->stream) != hipSuccess || hipGetLastError() != hipSuccess ||
        (H && hipMemcpy(H, dH, n6 * n6 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
        (g6N && hipMemcpy(g6N, dg, n6 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
      rc = fail("ba_pgraph_get_system: device error");
  }
  (void)hipFree(dH);
  (void)hipFree(dg);
  return rc;
}

int ba_pgraph_info(ba_pgraph *g, int64_t out8[8]) {
  if (!g || !out8) return fail("ba_pgraph_info: bad argument");
  out8[0] = g->d.N;
  out8[1] = g->F;
  out8[2] = g->d.nblk;
  out8[3] = g->nb;
  out8[4] = g->ncb;
  out8[5] = g->sched.nlev;
  out8[6] = (int64_t)g->image_bytes;
  out8[7] = g->bad_pivots;
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
  PgCovCall c;
  c.n_pose_sel = n_pose_sel;
  c.pose_sel = pose_sel;
  c.cov_pose36 = cov_pose36;
  c.n_entry = n_pair;
  c.entry_j = pair_j;
  c.entry_k = pair_k;
  c.cov_cross36 = n_pair > 0 ? cov_cross36 : nullptr;
  c.cov_rel36 = cov_rel36;
  return pg_cov_run(g, "ba_pgraph_covariance", c, dropped_pivots);
}

int ba_pgraph_gate(ba_pgraph *g, int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k, const double *Z12,
                   const double *Omega36, double *d2, double *r6, double *innov36, int64_t *dropped_pivots) {
  if (!g) return fail("ba_pgraph_gate: null graph");
  if (ba_pgraph_cov_check(g->n_pose, g->fixed.data(), 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, n_cand,
                          cand_j, cand_k, Z12, Omega36, d2))
    return -1;
  PgCovCall c;
  c.n_entry = n_cand;
  c.entry_kind = ba::kPgCovCand;
  c.entry_j = cand_j;
  c.entry_k = cand_k;
  c.Z12 = Z12;
  c.Omega36 = Omega36;
  c.d2 = d2;
  c.r6 = n_cand > 0 ? r6 : nullptr;
  c.innov36 = n_cand > 0 ? innov36 : nullptr;
  return pg_cov_run(g, "ba_pgraph_gate", c, dropped_pivots);
}

int ba_pgraph_cov_info(ba_pgraph *g, int64_t out4[4]) {
  if (!g || !out4) return fail("ba_pgraph_cov_info: bad argument");
  const int bw = ba::cov_batch_cols(g->d.npad, g->h->knobs.run);
  out4[0] = bw;
  out4[1] = ba::kCovGroupCols;
  out4[2] = g->cov_batches;
  out4[3] = (int64_t)g->d.npad * bw * (int64_t)sizeof(double);
  return 0;
}

int ba_pgraph_last_ms(ba_pgraph *g, double *ms) {
  if (!g || !ms) return fail("ba_pgraph_last_ms: bad argument");
  *ms = g->last_ms;
  return 0;
}

}  // extern "C"
