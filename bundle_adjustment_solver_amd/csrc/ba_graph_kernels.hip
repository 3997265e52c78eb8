// ba_graph_kernels.hip — the kernels of the pose graphs, each written once and instantiated for
// the SE(3) graph (ba_pgraph_*) and the Sim(3) graph (ba_sim3_*; §6o, §6p)
// over the group's struct of ba_graph_fn.h.  Levenberg-Marquardt over relative factors alone,
// chi2 = sum_f r_f^T Omega_f r_f; the factor arithmetic is defined once, in ba_rel_fn.h,
// ba_sim3_fn.h and ba_factor_fn.h, the linear solve is the level-scheduled tile Cholesky of
// ba_dense.hip.  With W the group's tangent width:
//   k_graph_lin       kFpb factors per workgroup: E, r and Ad per factor into LDS, then one thread
//                     per element of Omega Ad, Omega r, Ad^T Omega Ad, Ad^T Omega r; the record of
//                     a factor (2 W W + 2 W doubles) leaves in runs of W W / W consecutive doubles
//                     (Ad and r never leave LDS); the workgroup's chi-square partial.  Cost-only
//                     mode: the partial alone (and, on the plain Sim(3) kernel, s_f per factor for
//                     ba_sim3_factor_report)
//   k_graph_assemble  one thread per element of H_jj / g_j walks the pose's list, one per element
//                     of a coupled block the block's list, in input order; H + lambda diag(H) and
//                     g go straight into the dense image, diag(H) and g are kept for pred
//   k_graph_trial     one thread per optimisable pose: X_j <- exp(x_j) X_j into the other pose
//                     buffer; partials of sum |x_j| and of pred.  One specialisation per group
//   k_pg_control      one workgroup: the sums, rho, status, lambda, the buffer swap, the stop test,
//                     the log row.  It knows nothing of a pose's width: one kernel for both groups
// One writer per element, fixed trees, no floating-point atomics: the same bits run to run.
// Robust kernels (ba_pgraph_set_robust, ba_sim3_set_robust; §6l, §6p): the second instantiations
// of k_graph_lin and k_graph_assemble, with sum rho(s) for chi-square and w Omega for Omega; a graph
// whose kinds are all 0 launches the plain ones, in which every robust line is compiled out.
// Every variant is an instantiation of a __global__ template.  A __device__ body inlined into
// several __global__ wrappers is NOT the same thing to the compiler: its early returns become
// branches to a join, and the plain Sim(3) linearisation came out with other scalar registers that
// way (46 for 48 SGPRs).  The instantiations below have the instruction streams and the resources
// of the kernels they replace (profiles/graph_kernels_v1.txt).
// The kernel table (ba_device.h) lists the instantiations under the ids and names they had as
// separate kernels: k_pg_lin, k_s3_lin_robust, ...
//
// Covariance blocks and the chi-square gate for loop-closure candidates (ba_pgraph_covariance /
// ba_pgraph_gate, ba_sim3_covariance / ba_sim3_gate; §6m, §6p): k_graph_cov_rhs and
// k_graph_cov_solve<G, NB>.  With H = L L^T the tile Cholesky that dense_factor_solve leaves in the
// graph's dense image at lambda = 0, Sigma = H^-1 and Z_j = L^-1 E_j (the W identity columns of
// pose j):
//   Sigma_jj = Z_j^T Z_j,   Sigma_jk = Z_j^T Z_k.
// One wave owns 16 right-hand sides: the columns of one pose in 0..W-1, of a second in W..2W-1 (at
// W = 7 columns 14 and 15 stay zero).  It sweeps them with cov_sweep<NB> (ba_cov_sweep.h: the sweep
// of ba_covariance's k_cov_solve), and its 16x16 Gram matrix holds Sigma_jj, Sigma_kk and Sigma_jk
// at once.  What the wave does with them is the epilogue, through LDS:
//   kind 0 (two selected poses)  the two diagonal blocks
//   kind 1 (a pair j, k)         Sigma_jk (if asked for) and, with E = X_j X_k^-1 at the current
//                                poses and Ad = Ad(E),
//                                Sigma_E = Sigma_jj - Sigma_jk Ad^T - Ad Sigma_kj + Ad Sigma_kk Ad^T
//   kind 2 (a candidate)         also r = log(E Z^-1), P = Sigma_E + Omega_z^-1 and
//                                d2 = r^T P^-1 r: two W x W Cholesky solves in plain fp64; a pivot of
//                                P that is not positive gives d2 = NaN
// A fixed member of a pair has no column: its blocks of the Gram matrix are exactly zero and the
// formula above is the reduced one.  No atomics, one writer per element, every sum in a fixed
// order: a block has the same bits run to run, in any selection and any batch split.
//
// The host side is the graph driver of ba_graph.hip; it reaches the launchers at the end of this
// file through the GraphSpec of a kind (ba_pgraph.hip, ba_sim3.hip).
#include <type_traits>

#include "ba_cov_sweep.h"
#include "ba_device.h"
#include "ba_graph_fn.h"
#include "ba_robust_fn.h"

namespace ba {
namespace {

constexpr int kGraphBlock = 256;
inline int graph_cdiv(int64_t a, int b) { return (int)((a + b - 1) / b); }

// (rho(s) and w = rho'(s) of one factor: pg_rho of ba_robust_fn.h)

// The last argument of a linearisation kernel: the robust record, or what the group's plain kernel
// has in its place (GraphNoArg; Sim3Report with the array of ba_sim3_factor_report)
template <class G, bool kRobust>
using GraphLinArg = typename std::conditional<kRobust, PgRobust, typename G::LinPlain>::type;

// w of the robust kernel is computed once per factor by the thread that has s, rides through LDS
// (sW) to the element threads of the second phase, and is folded into Omega Ad and Omega r there:
// the record is linear in Omega, so Ad^T Omega Ad and Ad^T Omega r of the third phase carry it too.
template <class G, bool kRobust>
__global__ __launch_bounds__(kGraphBlock) void k_graph_lin(PgDev p, int cost_only, GraphLinArg<G, kRobust> rb) {
  constexpr int W = G::W, WW = W * W, kEl = WW + W, kFpb = G::kFpb, kAdS = G::kAdS, kRS = G::kRS;
  __shared__ double sAd[kFpb * kAdS], sOA[kFpb * kAdS], sR[kFpb * kRS], sOr[kFpb * kRS];
  __shared__ double sm[4];
  __shared__ double sW[kRobust ? kFpb : 1];
  const PgCtrl *c = p.ctrl;
  if (c->done) return;
  if (!cost_only && !c->relin) return;  // a rejected step: the records still belong to the accepted poses
  const double *P = p.poses[cost_only == 1 ? c->cur ^ 1 : c->cur];
  const int f0 = blockIdx.x * kFpb;
  const int nf = min(kFpb, p.F - f0);
  const int tid = threadIdx.x;
  const double *val = p.val + (size_t)f0 * G::kVal;
  double q = 0.0;
  if (tid < nf) {
    const int4 jk = p.jk[f0 + tid];
    typename G::Elem E;
    double rr[W];
    G::rel(jk.x, jk.y, P, E);
    const double *Z = val + (size_t)tid * G::kVal, *Om = Z + G::kPose;
    G::res(E, Z, rr);
    q = factor_quad<W>(Om, rr);
    if constexpr (std::is_same<GraphLinArg<G, kRobust>, Sim3Report>::value) {
      if (rb.rep) rb.rep[f0 + tid] = q;
    }
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
      G::Ad(E, sAd + tid * kAdS);
#pragma unroll
      for (int a = 0; a < W; ++a) sR[tid * kRS + a] = rr[a];
    }
  }
  if (!cost_only) {
    double *rec = p.rec + (size_t)f0 * G::kRec;
    __syncthreads();
    // OA = Omega Ad and Or = Omega r, one thread per element
    for (int e = tid; e < kEl * nf; e += kGraphBlock) {
      const int f = e / kEl, k = e - kEl * f;
      const double *Om = val + (size_t)f * G::kVal + G::kPose;
      if (k < WW) {
        double acc = factor_OA<W>(Om, sAd + f * kAdS, k);
        if constexpr (kRobust) acc *= sW[f];  // the record is linear in Omega: w Omega from here on
        sOA[f * kAdS + k] = acc;
        rec[(size_t)f * G::kRec + G::kOA + k] = acc;
      } else {
        const int a = k - WW;
        double acc = factor_Or<W>(Om, sR + f * kRS, a);
        if constexpr (kRobust) acc *= sW[f];
        sOr[f * kRS + a] = acc;
        rec[(size_t)f * G::kRec + G::kOr + a] = acc;
      }
    }
    __syncthreads();
    // Bk = Ad^T OA and gk = Ad^T Or, for the factors whose k is optimisable
    for (int e = tid; e < kEl * nf; e += kGraphBlock) {
      const int f = e / kEl, k = e - kEl * f;
      if (p.jk[f0 + f].w < 0) continue;
      if (k < WW) {
        rec[(size_t)f * G::kRec + G::kBk + k] = factor_Bk<W>(sAd + f * kAdS, sOA + f * kAdS, k);
      } else {
        const int a = k - WW;
        rec[(size_t)f * G::kRec + G::kGk + a] = factor_gk<W>(sAd + f * kAdS, sOr + f * kRS, a);
      }
    }
  }
  const double tot = block_sum(q, sm);
  if (tid == 0) p.part[cost_only ? 1 : 0][blockIdx.x] = tot;
}

// Arg...: what follows gout.  PgRobust makes the robust kernel; the plain kernel has GraphNoArg
// there or nothing, as the group's argument list has had it (G::kAssemblePlainArg).
template <class G, class... Arg>
__global__ __launch_bounds__(kGraphBlock) void k_graph_assemble(PgDev p, double *Hout, double *gout, Arg... arg) {
  constexpr int W = G::W, WW = W * W, kEl = WW + W;
  constexpr bool kRobust = (std::is_same<Arg, PgRobust>::value || ...);
  const PgCtrl *c = p.ctrl;
  if (c->done) return;
  const int64_t e = (int64_t)blockIdx.x * kGraphBlock + threadIdx.x;
  const int64_t nd = (int64_t)kEl * p.N;
  const size_t nW = (size_t)W * p.N;
  if (e < nd) {
    const int j = (int)(e / kEl), q = (int)(e - (int64_t)kEl * j);
    // (the two walks are rel_walk_pose / rel_walk_block of ba_rel_fn.h written out: calling
    // them measured 2 % slower here, see profiles/rel_shared_v1.txt)
    const int l1 = p.pptr[j + 1];
    double acc = 0.0;
    for (int l = p.pptr[j]; l < l1; ++l) {
      const int w = p.plist[l], f = w >> 1;
      const double *rec = p.rec + (size_t)f * G::kRec;
      if (q < WW)
        if constexpr (kRobust)  // H_jj += w Omega: the one term that is not read from the records
          acc += (w & 1) ? rec[G::kBk + q] : (arg.w[f], ...) * p.val[(size_t)f * G::kVal + G::kPose + q];
        else
          acc += (w & 1) ? rec[G::kBk + q] : p.val[(size_t)f * G::kVal + G::kPose + q];
      else
        acc += (w & 1) ? rec[G::kGk + q - WW] : -rec[G::kOr + q - WW];
    }
    const int pc = p.pose_col[j];
    if (q < WW) {
      const int rw = q / W, cc = q - W * rw;
      if (Hout) {
        Hout[((size_t)W * j + rw) * nW + (size_t)W * j + cc] = acc;
      } else {
        if (rw == cc) {
          p.dH[W * j + rw] = acc;
          acc = acc + c->lambda * acc;
        }
        if (rw >= cc) p.L[(size_t)(pc + cc) * p.ld + pc + rw] = acc;
      }
    } else {
      const int r = q - WW;
      if (Hout) {
        gout[W * j + r] = acc;
      } else {
        p.g[W * j + r] = acc;
        p.L[(size_t)(pc + r) * p.ld + p.npad] = acc;  // the right-hand side rides as row npad
      }
    }
    return;
  }
  const int64_t eb = e - nd;
  if (eb >= (int64_t)WW * p.nblk) return;
  const int b = (int)(eb / WW), rc = (int)(eb - (int64_t)WW * b), r = rc / W, cc = rc - W * r;
  const int2 hl = p.blk[b];
  const int l1 = p.bptr[b + 1];
  double acc = 0.0;
  for (int l = p.bptr[b]; l < l1; ++l) {
    const int w = p.blist[l], f = w >> 1;
    acc -= p.rec[(size_t)f * G::kRec + G::kOA + ((w & 1) ? cc * W + r : rc)];
  }
  if (Hout) {
    Hout[((size_t)W * hl.x + r) * nW + (size_t)W * hl.y + cc] = acc;
    Hout[((size_t)W * hl.y + cc) * nW + (size_t)W * hl.x + r] = acc;
    return;
  }
  // element (r, cc) of H_hi,lo; where the column map puts it above the diagonal it is stored
  // transposed, so that the lower triangle of the image is complete
  const int row = p.pose_col[hl.x] + r, col = p.pose_col[hl.y] + cc;
  p.L[row > col ? (size_t)col * p.ld + row : (size_t)row * p.ld + col] = acc;
}

// k_graph_trial is the one kernel with a text per group.  The groups differ in the retraction, in
// how a thread holds x_j and in how it sums |x_j|^2, and every shared form that was tried (the
// retraction, or the whole step of one pose, as a function of the group's struct) gave other
// instructions than the kernels had: at best the same ones with the operands of some adds and
// multiplies exchanged (profiles/graph_kernels_v1.txt).  So each specialisation is the text its
// group has had, and only the launcher is shared.
template <class G>
__global__ void k_graph_trial(PgDev p);

template <>
__global__ __launch_bounds__(kGraphBlock) void k_graph_trial<Se3Graph>(PgDev p) {
  __shared__ double sm[8];
  const PgCtrl *c = p.ctrl;
  if (c->done) return;
  const int j = blockIdx.x * kGraphBlock + threadIdx.x;
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

template <>
__global__ __launch_bounds__(kGraphBlock) void k_graph_trial<Sim3Graph>(PgDev p) {
  __shared__ double sm[8];
  const PgCtrl *c = p.ctrl;
  if (c->done) return;
  const int j = blockIdx.x * kGraphBlock + threadIdx.x;
  double sx = 0.0, pr = 0.0;
  if (j < p.N) {
    double xj[7], dS[13], So[13];
#pragma unroll
    for (int r = 0; r < 7; ++r) xj[r] = p.x[(size_t)7 * j + r];
    sim3_exp(xj, dS);
    const int ps = p.opt_pose[j];
    sim3_mul(dS, p.poses[c->cur] + (size_t)ps * 13, So);
    double *out = p.poses[c->cur ^ 1] + (size_t)ps * 13;
#pragma unroll
    for (int r = 0; r < 13; ++r) out[r] = So[r];
    double gx = 0.0, dx = 0.0, n2 = 0.0;
#pragma unroll
    for (int r = 0; r < 7; ++r) {
      gx += p.g[7 * j + r] * xj[r];
      dx += (xj[r] * p.dH[7 * j + r]) * xj[r];
      n2 += xj[r] * xj[r];
    }
    pr = gx + c->lambda * dx;  // pred = g^T x + lambda x^T diag(H) x
    sx = sqrt(n2);
  }
  block_sum2(sx, pr, sm);
  if (threadIdx.x == 0) {
    p.tpart[2 * blockIdx.x + 0] = sx;
    p.tpart[2 * blockIdx.x + 1] = pr;
  }
}

__global__ __launch_bounds__(kGraphBlock) void k_pg_control(PgDev p, int mode) {
  __shared__ double sm[8];
  PgCtrl *c = p.ctrl;
  if (c->done) return;
  double a = 0.0, t = 0.0, sx = 0.0, pr = 0.0;
  for (int k = threadIdx.x; k < p.n_part; k += kGraphBlock) {
    a += p.part[0][k];
    t += p.part[1][k];
  }
  block_sum2(a, t, sm);
  if (mode == 1) {
    if (threadIdx.x == 0) c->aux = t;
    return;
  }
  for (int k = threadIdx.x; k < p.n_tpart; k += kGraphBlock) {
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

// ---- covariance blocks and the gate ---------------------------------------------------------

// identity columns of the group's optimisable members into the (zeroed) workspace
template <class G>
__global__ __launch_bounds__(64) void k_graph_cov_rhs(const PgCovGroup *__restrict__ groups, double *Zw, int bw,
                                                      const int *__restrict__ pose_col) {
  constexpr int W = G::W;
  const int lane = threadIdx.x;
  if (lane >= 2 * W) return;
  const int a = lane / W, r = lane - W * a;
  const int j = groups[blockIdx.x].opt[a];
  if (j >= 0) Zw[(size_t)(pose_col[j] + r) * bw + kCovGroupCols * blockIdx.x + W * a + r] = 1.0;
}

// In-place Cholesky of the W x W matrix A (row-major, LDS; the lower triangle is read and
// replaced by the factor); false at a pivot that is not positive.  One lane.
template <int W>
__device__ __forceinline__ bool cholw(double *A) {
  for (int c = 0; c < W; ++c) {
    double d = A[c * W + c];
    for (int m = 0; m < c; ++m) d -= A[c * W + m] * A[c * W + m];
    if (!(d > 0.0)) return false;
    const double s = sqrt(d);
    A[c * W + c] = s;
    for (int r = c + 1; r < W; ++r) {
      double v = A[r * W + c];
      for (int m = 0; m < c; ++m) v -= A[r * W + m] * A[c * W + m];
      A[r * W + c] = v / s;
    }
  }
  return true;
}
// x <- (L L^T)^-1 x for the factor cholw left in A (x: W doubles in LDS, stride xs).  One lane.
template <int W>
__device__ __forceinline__ void cholw_solve(const double *A, double *x, const int xs) {
  for (int r = 0; r < W; ++r) {
    double v = x[r * xs];
    for (int m = 0; m < r; ++m) v -= A[r * W + m] * x[m * xs];
    x[r * xs] = v / A[r * W + r];
  }
  for (int r = W - 1; r >= 0; --r) {
    double v = x[r * xs];
    for (int m = r + 1; m < W; ++m) v -= A[m * W + r] * x[m * xs];
    x[r * xs] = v / A[r * W + r];
  }
}

template <class G, int NB>
__global__ __launch_bounds__(64) void k_graph_cov_solve(const double *__restrict__ L, int ld,
                                                        const double *__restrict__ Ldiag, int ncb,
                                                        const int *__restrict__ trow_ptr,
                                                        const int *__restrict__ trow,
                                                        const PgCovGroup *__restrict__ groups, double *Zw, int bw,
                                                        const double *__restrict__ poses,
                                                        const double *__restrict__ cand_val, GraphCovOut out) {
  constexpr int W = G::W, WW = W * W;
  __shared__ double sG[256];                       // the Gram matrix, row-major
  __shared__ double sAd[WW], sA[WW], sS[WW], sW[WW], sP[WW], sr[W], sy[W];
  __shared__ int ok;
  const PgCovGroup g = groups[blockIdx.x];
  const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4;
  double *Zc = Zw + kCovGroupCols * blockIdx.x + lr;  // this lane's column
  const cov_v4f64 Gm = cov_sweep<NB>(L, ld, Ldiag, ncb, trow_ptr, trow, g.t0, Zc, bw);
#pragma unroll
  for (int q = 0; q < 4; ++q) sG[(lk + 4 * q) * 16 + lr] = Gm[q];
  __syncthreads();
  if (g.kind == kPgCovPoses) {  // the diagonal blocks
    for (int e = lane; e < 2 * WW; e += 64) {
      const int a = e / WW, q = e - WW * a, r = q / W, c = q - W * r;
      if (g.slot[a] >= 0) out.pose[(size_t)g.slot[a] * WW + q] = sG[(W * a + r) * 16 + W * a + c];
    }
    return;
  }
  const size_t slot = (size_t)g.slot[0];
  // a candidate's Z and Omega_z (W x W, mirrored by the host)
  const double *val = g.kind == kPgCovCand ? cand_val + slot * G::kVal : nullptr;
  if (lane == 0) {
    typename G::Elem E;
    G::rel(g.pose[0], g.pose[1], poses, E);
    G::Ad(E, sAd);
    if (g.kind == kPgCovCand) {
      double rr[W];
      G::res(E, val, rr);
#pragma unroll
      for (int a = 0; a < W; ++a) sr[a] = sy[a] = rr[a];
    }
  }
  __syncthreads();
  const int r0 = lane / W, c0 = lane - W * r0;  // lanes 0..WW-1: one element of a W x W block each
  if (lane < WW) {  // A = Ad Sigma_kk
    double acc = 0.0;
    for (int m = 0; m < W; ++m) acc += sAd[r0 * W + m] * sG[(W + m) * 16 + W + c0];
    sA[lane] = acc;
  }
  __syncthreads();
  if (lane < WW) {
    // element (r0, c0) of Sigma_E from the expression of its lower-triangle twin, so that the
    // block is symmetric to the bit (Sigma_kj[m][c] = Sigma_jk[c][m], the Gram matrix is)
    const int a = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
    double t1 = 0.0, t2 = 0.0, t3 = 0.0;
    for (int m = 0; m < W; ++m) {
      t1 += sG[a * 16 + W + m] * sAd[c * W + m];
      t2 += sAd[a * W + m] * sG[c * 16 + W + m];
      t3 += sA[a * W + m] * sAd[c * W + m];
    }
    const double v = ((sG[a * 16 + c] - t1) - t2) + t3;
    sS[lane] = v;
    out.rel[slot * WW + lane] = v;
    if (out.cross) out.cross[slot * WW + lane] = sG[r0 * 16 + W + c0];
    if (g.kind == kPgCovCand) sW[lane] = val[G::kPose + lane];
  }
  if (g.kind != kPgCovCand) return;
  __syncthreads();
  // Omega_z^-1: the factor once, then one solve per identity column (lanes 0..W-1), in sP
  if (lane == 0) ok = cholw<W>(sW) ? 1 : 0;
  if (lane < WW) sP[lane] = r0 == c0 ? 1.0 : 0.0;
  __syncthreads();
  if (lane < W && ok) cholw_solve<W>(sW, sP + lane, W);
  __syncthreads();
  double pv = 0.0;
  if (lane < WW) {  // P = Sigma_E + Omega_z^-1, the inverse read from its lower-triangle twin
    const int a = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
    pv = sS[lane] + sP[a * W + c];
  }
  __syncthreads();
  if (lane < WW) {
    sW[lane] = pv;
    if (out.innov) out.innov[slot * WW + lane] = ok ? pv : __builtin_nan("");
  }
  if (lane < W && out.r) out.r[slot * W + lane] = sr[lane];
  __syncthreads();
  if (lane == 0) {
    double d2 = __builtin_nan("");
    if (ok && cholw<W>(sW)) {
      cholw_solve<W>(sW, sy, 1);
      d2 = 0.0;
      for (int a = 0; a < W; ++a) d2 += sr[a] * sy[a];
    }
    out.d2[slot] = d2;
  }
}

// the plain linearisation with its last argument given: launch_graph_lin and launch_s3_lin
template <class G>
void launch_lin_plain(const PgDev &p, int cost_only, typename G::LinPlain arg, hipStream_t s) {
  constexpr auto k = k_graph_lin<G, false>;
  BA_LAUNCH(G::kLin, k, dim3(p.n_part), dim3(kGraphBlock), s, p, cost_only, arg);
}

template <class G>
int assemble_grid(const PgDev &p) {
  return graph_cdiv((int64_t)(G::W * G::W + G::W) * p.N + (int64_t)(G::W * G::W) * p.nblk, kGraphBlock);
}

}  // namespace

template <class G>
void launch_graph_lin(const PgDev &p, int cost_only, hipStream_t s) {
  launch_lin_plain<G>(p, cost_only, typename G::LinPlain{}, s);
}
void launch_s3_lin(const PgDev &p, int cost_only, double *rep, hipStream_t s) {
  launch_lin_plain<Sim3Graph>(p, cost_only, Sim3Report{rep}, s);
}
template <class G>
void launch_graph_lin_robust(const PgDev &p, const PgRobust &rb, int cost_only, hipStream_t s) {
  constexpr auto k = k_graph_lin<G, true>;
  BA_LAUNCH(G::kLinRobust, k, dim3(p.n_part), dim3(kGraphBlock), s, p, cost_only, rb);
}
template <class G>
void launch_graph_assemble(const PgDev &p, double *Hout, double *gout, hipStream_t s) {
  if constexpr (G::kAssemblePlainArg) {
    constexpr auto k = k_graph_assemble<G, GraphNoArg>;
    BA_LAUNCH(G::kAssemble, k, dim3(assemble_grid<G>(p)), dim3(kGraphBlock), s, p, Hout, gout, GraphNoArg{});
  } else {
    constexpr auto k = k_graph_assemble<G>;
    BA_LAUNCH(G::kAssemble, k, dim3(assemble_grid<G>(p)), dim3(kGraphBlock), s, p, Hout, gout);
  }
}
template <class G>
void launch_graph_assemble_robust(const PgDev &p, const PgRobust &rb, double *Hout, double *gout, hipStream_t s) {
  constexpr auto k = k_graph_assemble<G, PgRobust>;
  BA_LAUNCH(G::kAssembleRobust, k, dim3(assemble_grid<G>(p)), dim3(kGraphBlock), s, p, Hout, gout, rb);
}
template <class G>
void launch_graph_trial(const PgDev &p, hipStream_t s) {
  constexpr auto k = k_graph_trial<G>;
  BA_LAUNCH(G::kTrial, k, dim3(p.n_tpart), dim3(kGraphBlock), s, p);
}
void launch_pg_control(const PgDev &p, int mode, hipStream_t s) {
  BA_LAUNCH(K_PG_CONTROL, k_pg_control, dim3(1), dim3(kGraphBlock), s, p, mode);
}

template <class G>
void launch_graph_cov_batch(const PgDev &p, const double *Ldiag, int nb, int ncb, const double *poses,
                            const int *trow_ptr, const int *trow, const PgCovGroup *groups, int ng,
                            const double *cand_val, double *Zw, int bw, const GraphCovOut &out, hipStream_t s) {
  if (ng <= 0) return;
  (void)hipMemsetAsync(Zw, 0, (size_t)p.npad * bw * sizeof(double), s);
  hipLaunchKernelGGL(k_graph_cov_rhs<G>, dim3(ng), dim3(64), 0, s, groups, Zw, bw, p.pose_col);
  constexpr auto k32 = k_graph_cov_solve<G, 32>, k64 = k_graph_cov_solve<G, 64>;
  if (nb == 32)
    hipLaunchKernelGGL(k32, dim3(ng), dim3(64), 0, s, p.L, p.ld, Ldiag, ncb, trow_ptr, trow, groups, Zw, bw, poses,
                       cand_val, out);
  else
    hipLaunchKernelGGL(k64, dim3(ng), dim3(64), 0, s, p.L, p.ld, Ldiag, ncb, trow_ptr, trow, groups, Zw, bw, poses,
                       cand_val, out);
}

// the launchers of both groups, for the GraphSpec of ba_pgraph.hip and of ba_sim3.hip
#define BA_GRAPH_LAUNCHERS(G)                                                                                        \
  template void launch_graph_lin<G>(const PgDev &, int, hipStream_t);                                                \
  template void launch_graph_lin_robust<G>(const PgDev &, const PgRobust &, int, hipStream_t);                       \
  template void launch_graph_assemble<G>(const PgDev &, double *, double *, hipStream_t);                            \
  template void launch_graph_assemble_robust<G>(const PgDev &, const PgRobust &, double *, double *, hipStream_t);   \
  template void launch_graph_trial<G>(const PgDev &, hipStream_t);                                                   \
  template void launch_graph_cov_batch<G>(const PgDev &, const double *, int, int, const double *, const int *,      \
                                          const int *, const PgCovGroup *, int, const double *, double *, int,      \
                                          const GraphCovOut &, hipStream_t);
BA_GRAPH_LAUNCHERS(Se3Graph)
BA_GRAPH_LAUNCHERS(Sim3Graph)
#undef BA_GRAPH_LAUNCHERS

}  // namespace ba
