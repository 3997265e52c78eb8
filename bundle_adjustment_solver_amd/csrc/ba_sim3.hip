// ba_sim3.hip — Sim(3) pose-graph optimisation (ba_sim3_*, include/ba_hip.h):
// Levenberg-Marquardt over relative-similarity factors alone, 7 DoF per pose, chi2 = sum_f
// r_f^T Omega_f r_f.  The 7-DoF loop closing of a monocular map; the reference project has no
// counterpart, the definition is the comment of ba_sim3_create.  The factor arithmetic is
// defined once, in ba_sim3_fn.h; the lists are the pose graph's (ba_pgraph_host.h), the linear
// solve is the level-scheduled tile Cholesky of ba_dense.hip with seven columns per pose, and
// the controller is k_pg_control of ba_pgraph.hip, which knows nothing of a pose's width.
// Three kernels of its own:
//   k_s3_lin       kS3Fpb factors per workgroup: E, r and Ad7 per factor into LDS, then one
//                  thread per element of Omega Ad, Omega r, Ad^T Omega Ad, Ad^T Omega r; the
//                  112-double record of a factor leaves in runs of 49 / 7 consecutive doubles
//                  (Ad and r never leave LDS); the workgroup's chi-square partial.  Cost-only
//                  mode: the partial alone (and s_f per factor for ba_sim3_factor_report)
//   k_s3_assemble  one thread per element of H_jj / g_j walks the pose's list, one per element
//                  of a coupled block the block's list, in input order; H + lambda diag(H) and
//                  g go straight into the dense image, diag(H) and g are kept for pred
//   k_s3_trial     one thread per optimisable pose: S_j <- sim3_exp(x_j) S_j into the other pose
//                  buffer; partials of sum |x_j| and of pred
// One writer per element, fixed trees, no floating-point atomics: the same bits run to run.
// Robust kernels (ba_sim3_set_robust): k_s3_lin_robust and k_s3_assemble_robust
// are the two kernels with sum rho(s) for chi-square and w Omega for Omega: k_s3_lin written out a
// second time, k_s3_assemble instantiated a second time (the comment before k_s3_lin_robust says
// why the two differ); a graph whose kinds are all 0 launches the plain ones.
// Covariance blocks and the gate (ba_sim3_covariance / ba_sim3_gate): the host side
// is here (s3_cov_run: the solve's launches at lambda = 0, then column batches), the groups are
// the pose graph's (ba_pgraph_host.h), the validation in ba_sim3_host.h, the kernels in
// ba_sim3_cov.hip.
#include <cstddef>
#include <cstring>
#include <type_traits>

#include "ba_handle.h"
#include "ba_sim3_host.h"
#include "ba_device_fn.h"
#include "ba_robust_fn.h"
#include "ba_sim3_fn.h"

namespace ba {
namespace {

constexpr int kS3Block = 256;
// the per-factor LDS rows keep their natural strides: 49 and 7 doubles are odd, so the 32
// factor threads of the first phase write 32 different bank pairs, and the element threads of
// the later phases read and write consecutive doubles
constexpr int kS3AdS = 49, kS3RS = 7;
inline int s3_cdiv(int64_t a, int b) { return (int)((a + b - 1) / b); }

__global__ __launch_bounds__(kS3Block) void k_s3_lin(PgDev p, int cost_only, double *rep) {
  __shared__ double sAd[kS3Fpb * kS3AdS], sOA[kS3Fpb * kS3AdS], sR[kS3Fpb * kS3RS], sOr[kS3Fpb * kS3RS];
  __shared__ double sm[4];
  const PgCtrl *c = p.ctrl;
  if (c->done) return;
  if (!cost_only && !c->relin) return;  // a rejected step: the records still belong to the accepted poses
  const double *P = p.poses[cost_only == 1 ? c->cur ^ 1 : c->cur];
  const int f0 = blockIdx.x * kS3Fpb;
  const int nf = min(kS3Fpb, p.F - f0);
  const int tid = threadIdx.x;
  const double *val = p.val + (size_t)f0 * kS3Val;
  double q = 0.0;
  if (tid < nf) {
    const int4 jk = p.jk[f0 + tid];
    double E[13], rr[7];
    sim3_E(jk.x, jk.y, P, E);
    const double *Z = val + (size_t)tid * kS3Val, *Om = Z + 13;
    sim3_res(E, Z, rr);
    q = sim3_quad(Om, rr);
    if (rep) rep[f0 + tid] = q;
    if (!cost_only) {  // r and Ad
      sim3_Ad(E, sAd + tid * kS3AdS);
#pragma unroll
      for (int a = 0; a < 7; ++a) sR[tid * kS3RS + a] = rr[a];
    }
  }
  if (!cost_only) {
    double *rec = p.rec + (size_t)f0 * kS3Rec;
    __syncthreads();
    // OA = Omega Ad and Or = Omega r, one thread per element
    for (int e = tid; e < 56 * nf; e += kS3Block) {
      const int f = e / 56, k = e - 56 * f;
      const double *Om = val + (size_t)f * kS3Val + 13;
      if (k < 49) {
        const double acc = sim3_OA(Om, sAd + f * kS3AdS, k);
        sOA[f * kS3AdS + k] = acc;
        rec[(size_t)f * kS3Rec + kS3OA + k] = acc;
      } else {
        const int a = k - 49;
        const double acc = sim3_Or(Om, sR + f * kS3RS, a);
        sOr[f * kS3RS + a] = acc;
        rec[(size_t)f * kS3Rec + kS3Or + a] = acc;
      }
    }
    __syncthreads();
    // Bk = Ad^T OA and gk = Ad^T Or, for the factors whose k is optimisable
    for (int e = tid; e < 56 * nf; e += kS3Block) {
      const int f = e / 56, k = e - 56 * f;
      if (p.jk[f0 + f].w < 0) continue;
      if (k < 49) {
        rec[(size_t)f * kS3Rec + kS3Bk + k] = sim3_Bk(sAd + f * kS3AdS, sOA + f * kS3AdS, k);
      } else {
        const int a = k - 49;
        rec[(size_t)f * kS3Rec + kS3Gk + a] = sim3_gk(sAd + f * kS3AdS, sOr + f * kS3RS, a);
      }
    }
  }
  const double tot = block_sum(q, sm);
  if (tid == 0) p.part[cost_only ? 1 : 0][blockIdx.x] = tot;
}

// The robust record as an argument of the assembly's body: an empty struct for the plain kernel
struct S3NoRobust {};
template <bool kRobust>
using S3RobustArg = typename std::conditional<kRobust, PgRobust, S3NoRobust>::type;

// The body of k_s3_assemble and k_s3_assemble_robust, forced inline into each.  kRobust = false is
// the kernel of §6o: the robust line is compiled out, and the plain kernel keeps its instructions
// (its assembly was compared with the parent commit's; k_s3_lin did NOT survive this form, see below).
template <bool kRobust>
__device__ __forceinline__ void s3_assemble_body(const PgDev &p, double *Hout, double *gout,
                                                 const S3RobustArg<kRobust> &rb) {
  const PgCtrl *c = p.ctrl;
  if (c->done) return;
  const int64_t e = (int64_t)blockIdx.x * kS3Block + threadIdx.x;
  const int64_t nd = (int64_t)56 * p.N;
  const size_t n7 = (size_t)7 * p.N;
  if (e < nd) {
    const int j = (int)(e / 56), q = (int)(e - (int64_t)56 * j);
    const int l1 = p.pptr[j + 1];
    double acc = 0.0;
    for (int l = p.pptr[j]; l < l1; ++l) {
      const int w = p.plist[l], f = w >> 1;
      const double *rec = p.rec + (size_t)f * kS3Rec;
      if (q < 49)
        if constexpr (kRobust)  // H_jj += w Omega: the one term that is not read from the records
          acc += (w & 1) ? rec[kS3Bk + q] : rb.w[f] * p.val[(size_t)f * kS3Val + 13 + q];
        else
          acc += (w & 1) ? rec[kS3Bk + q] : p.val[(size_t)f * kS3Val + 13 + q];
      else
        acc += (w & 1) ? rec[kS3Gk + q - 49] : -rec[kS3Or + q - 49];
    }
    const int pc = p.pose_col[j];
    if (q < 49) {
      const int rw = q / 7, cc = q - 7 * rw;
      if (Hout) {
        Hout[((size_t)7 * j + rw) * n7 + (size_t)7 * j + cc] = acc;
      } else {
        if (rw == cc) {
          p.dH[7 * j + rw] = acc;
          acc = acc + c->lambda * acc;
        }
        if (rw >= cc) p.L[(size_t)(pc + cc) * p.ld + pc + rw] = acc;
      }
    } else {
      const int r = q - 49;
      if (Hout) {
        gout[7 * j + r] = acc;
      } else {
        p.g[7 * j + r] = acc;
        p.L[(size_t)(pc + r) * p.ld + p.npad] = acc;  // the right-hand side rides as row npad
      }
    }
    return;
  }
  const int64_t eb = e - nd;
  if (eb >= (int64_t)49 * p.nblk) return;
  const int b = (int)(eb / 49), rc = (int)(eb - (int64_t)49 * b), r = rc / 7, cc = rc - 7 * r;
  const int2 hl = p.blk[b];
  const int l1 = p.bptr[b + 1];
  double acc = 0.0;
  for (int l = p.bptr[b]; l < l1; ++l) {
    const int w = p.blist[l], f = w >> 1;
    acc -= p.rec[(size_t)f * kS3Rec + kS3OA + ((w & 1) ? cc * 7 + r : rc)];
  }
  if (Hout) {
    Hout[((size_t)7 * hl.x + r) * n7 + (size_t)7 * hl.y + cc] = acc;
    Hout[((size_t)7 * hl.y + cc) * n7 + (size_t)7 * hl.x + r] = acc;
    return;
  }
  // element (r, cc) of H_hi,lo; where the column map puts it above the diagonal it is stored
  // transposed, so that the lower triangle of the image is complete
  const int row = p.pose_col[hl.x] + r, col = p.pose_col[hl.y] + cc;
  p.L[row > col ? (size_t)col * p.ld + row : (size_t)row * p.ld + col] = acc;
}

__global__ __launch_bounds__(kS3Block) void k_s3_assemble(PgDev p, double *Hout, double *gout) {
  s3_assemble_body<false>(p, Hout, gout, S3NoRobust{});
}
__global__ __launch_bounds__(kS3Block) void k_s3_assemble_robust(PgDev p, double *Hout, double *gout, PgRobust rb) {
  s3_assemble_body<true>(p, Hout, gout, rb);
}

// k_s3_lin_robust (ba_sim3_set_robust) is k_s3_lin written out a second time with
// sum rho(s) for chi-square and w Omega for Omega.  One body instantiated twice, as the assembly
// above has it, was tried for this kernel and dropped: the early returns of the inlined body
// become branches to a join, and the plain k_s3_lin came out with other scalar registers (46 for
// 48 SGPRs).  k_s3_lin above is the text of §6o, so a graph without a kernel runs the instructions
// it ran before.  AN EDIT TO ONE OF THE TWO LINEARISATION KERNELS BELONGS IN THE OTHER AS WELL.
// w is computed once per factor by the thread that has s, rides through LDS (sW) to the element
// threads of the second phase, and is folded into Omega Ad and Omega r there: the record is
// linear in Omega, so Ad^T Omega Ad and Ad^T Omega r of the third phase carry it too.
__global__ __launch_bounds__(kS3Block) void k_s3_lin_robust(PgDev p, int cost_only, PgRobust rb) {
  __shared__ double sAd[kS3Fpb * kS3AdS], sOA[kS3Fpb * kS3AdS], sR[kS3Fpb * kS3RS], sOr[kS3Fpb * kS3RS];
  __shared__ double sm[4];
  __shared__ double sW[kS3Fpb];
  const PgCtrl *c = p.ctrl;
  if (c->done) return;
  if (!cost_only && !c->relin) return;  // a rejected step: the records still belong to the accepted poses
  const double *P = p.poses[cost_only == 1 ? c->cur ^ 1 : c->cur];
  const int f0 = blockIdx.x * kS3Fpb;
  const int nf = min(kS3Fpb, p.F - f0);
  const int tid = threadIdx.x;
  const double *val = p.val + (size_t)f0 * kS3Val;
  double q = 0.0;
  if (tid < nf) {
    const int4 jk = p.jk[f0 + tid];
    double E[13], rr[7];
    sim3_E(jk.x, jk.y, P, E);
    const double *Z = val + (size_t)tid * kS3Val, *Om = Z + 13;
    sim3_res(E, Z, rr);
    q = sim3_quad(Om, rr);
    {  // the partial is sum rho(s); w rides through LDS to the element threads
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
      sim3_Ad(E, sAd + tid * kS3AdS);
#pragma unroll
      for (int a = 0; a < 7; ++a) sR[tid * kS3RS + a] = rr[a];
    }
  }
  if (!cost_only) {
    double *rec = p.rec + (size_t)f0 * kS3Rec;
    __syncthreads();
    // OA = Omega Ad and Or = Omega r, one thread per element
    for (int e = tid; e < 56 * nf; e += kS3Block) {
      const int f = e / 56, k = e - 56 * f;
      const double *Om = val + (size_t)f * kS3Val + 13;
      if (k < 49) {
        double acc = sim3_OA(Om, sAd + f * kS3AdS, k);
        acc *= sW[f];  // the record is linear in Omega: w Omega from here on
        sOA[f * kS3AdS + k] = acc;
        rec[(size_t)f * kS3Rec + kS3OA + k] = acc;
      } else {
        const int a = k - 49;
        double acc = sim3_Or(Om, sR + f * kS3RS, a);
        acc *= sW[f];
        sOr[f * kS3RS + a] = acc;
        rec[(size_t)f * kS3Rec + kS3Or + a] = acc;
      }
    }
    __syncthreads();
    // Bk = Ad^T OA and gk = Ad^T Or, for the factors whose k is optimisable
    for (int e = tid; e < 56 * nf; e += kS3Block) {
      const int f = e / 56, k = e - 56 * f;
      if (p.jk[f0 + f].w < 0) continue;
      if (k < 49) {
        rec[(size_t)f * kS3Rec + kS3Bk + k] = sim3_Bk(sAd + f * kS3AdS, sOA + f * kS3AdS, k);
      } else {
        const int a = k - 49;
        rec[(size_t)f * kS3Rec + kS3Gk + a] = sim3_gk(sAd + f * kS3AdS, sOr + f * kS3RS, a);
      }
    }
  }
  const double tot = block_sum(q, sm);
  if (tid == 0) p.part[cost_only ? 1 : 0][blockIdx.x] = tot;
}

__global__ __launch_bounds__(kS3Block) void k_s3_trial(PgDev p) {
  __shared__ double sm[8];
  const PgCtrl *c = p.ctrl;
  if (c->done) return;
  const int j = blockIdx.x * kS3Block + threadIdx.x;
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

}  // namespace

void launch_s3_lin(const PgDev &p, int cost_only, double *rep, hipStream_t s) {
  BA_LAUNCH(K_S3_LIN, k_s3_lin, dim3(p.n_part), dim3(kS3Block), s, p, cost_only, rep);
}
void launch_s3_assemble(const PgDev &p, double *Hout, double *gout, hipStream_t s) {
  const int grid = s3_cdiv((int64_t)56 * p.N + (int64_t)49 * p.nblk, kS3Block);
  BA_LAUNCH(K_S3_ASSEMBLE, k_s3_assemble, dim3(grid), dim3(kS3Block), s, p, Hout, gout);
}
void launch_s3_lin_robust(const PgDev &p, const PgRobust &rb, int cost_only, hipStream_t s) {
  BA_LAUNCH(K_S3_LIN_ROBUST, k_s3_lin_robust, dim3(p.n_part), dim3(kS3Block), s, p, cost_only, rb);
}
void launch_s3_assemble_robust(const PgDev &p, const PgRobust &rb, double *Hout, double *gout, hipStream_t s) {
  const int grid = s3_cdiv((int64_t)56 * p.N + (int64_t)49 * p.nblk, kS3Block);
  BA_LAUNCH(K_S3_ASSEMBLE_ROBUST, k_s3_assemble_robust, dim3(grid), dim3(kS3Block), s, p, Hout, gout, rb);
}
void launch_s3_trial(const PgDev &p, hipStream_t s) {
  BA_LAUNCH(K_S3_TRIAL, k_s3_trial, dim3(p.n_tpart), dim3(kS3Block), s, p);
}

}  // namespace ba

// ---- host side ------------------------------------------------------------------------------
using ba::fail;
using ba::Mem;

struct ba_sim3 {
  ba_handle *h = nullptr;
  int n_pose = 0;
  int64_t F = 0;
  std::vector<uint8_t> fixed;
  std::vector<double> Z, Om;  // the factor values as given (ba_sim3_update_values replaces one or both)
  ba::PgraphLists lists;
  ba::DenseSchedule sched;
  ba::DenseDev dd;
  ba::PgDev d{};
  ba::PgCtrl hc{};
  double *Ldiag = nullptr, *val = nullptr, *rep = nullptr;
  // robust kernels: the host copy as given, the device arrays (allocated by the first
  // ba_sim3_set_robust with a kernel or ba_sim3_factor_weights), and whether any kind is not 0
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
  int cov_batches = 0;          // column batches of the last ba_sim3_covariance / ba_sim3_gate
  hipEvent_t e0 = nullptr, e1 = nullptr;
  std::vector<void *> allocs;
};

namespace {

// what was allocated on the handle since `mark` belongs to the graph from here on
void adopt_allocs(ba_sim3 *g, size_t mark) {
  ba_handle *h = g->h;
  g->allocs.insert(g->allocs.end(), h->allocs.begin() + mark, h->allocs.end());
  h->allocs.resize(mark);
}

void free_graph(ba_sim3 *g) {
  for (void *p : g->allocs) (void)hipFree(p);
  if (g->e0) (void)hipEventDestroy(g->e0);
  if (g->e1) (void)hipEventDestroy(g->e1);
  delete g;
}

int push_ctrl(ba_sim3 *g) {
  HIP_TRY(hipMemcpyAsync(g->d.ctrl, &g->hc, sizeof(ba::PgCtrl), hipMemcpyHostToDevice, g->h->stream));
  return 0;
}
int pull_ctrl(ba_sim3 *g) {
  HIP_TRY(hipMemcpyAsync(&g->hc, g->d.ctrl, sizeof(ba::PgCtrl), hipMemcpyDeviceToHost, g->h->stream));
  HIP_TRY(hipStreamSynchronize(g->h->stream));
  return 0;
}
const int *done_flag(const ba_sim3 *g) {
  return (const int *)((const char *)g->d.ctrl + offsetof(ba::PgCtrl, done));
}

// the device side of a validated graph; on failure the caller frees what `g` holds
int build_device(ba_sim3 *g, const double *S13) {
  ba_handle *h = g->h;
  const ba::PgraphLists &l = g->lists;
  const ba::DenseKnobs &knobs = h->knobs.dense;
  ba::PgDev &d = g->d;
  const int N = l.N;
  // both tile orders, as ba_pgraph_create builds them
  ba::DenseSchedule cand[2];
  const int orders[2] = {32, 64};
  for (int k = 0; k < 2; ++k) {
    int ncb_k = 0;
    std::vector<uint8_t> adj;
    ba::sim3_tile_adjacency(l, orders[k], &ncb_k, &adj);
    if (knobs.full) std::fill(adj.begin(), adj.end(), 1);
    ba::build_dense_schedule(ncb_k, adj, knobs.natural, orders[k], cand[k], knobs.order);
  }
  g->sched = cand[ba::dense_pick_tile_order(cand[0], cand[1], knobs.nb)];
  const ba::DenseSchedule &sc = g->sched;
  const int nb = sc.nb, ppt = ba::dense_sim3_per_tile(nb), ncb = sc.ncb;
  g->nb = nb;
  g->ncb = ncb;
  d.n_pose = g->n_pose;
  d.N = N;
  d.F = (int)g->F;
  d.nblk = (int)(l.blk.size() / 2);
  d.n_part = (int)((g->F + ba::kS3Fpb - 1) / ba::kS3Fpb);
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
      return fail("ba_sim3_create: cannot allocate the dense image of " + std::to_string(d.npad) + " x " +
                  std::to_string(d.ld) + " doubles (" + std::to_string(g->image_bytes) + " bytes): " +
                  hipGetErrorString(e));
    }
    g->allocs.push_back((void *)d.L);
  }
  // seven columns per pose; the nb - 7 ppt columns at the end of a tile are padding (col_x < 0:
  // k_dense_init gives them a unit diagonal)
  std::vector<int> pose_col((size_t)N, 0), col_x((size_t)d.npad, -1);
  for (int j = 0; j < N; ++j) {
    const int c0 = sc.pos_of_tile[j / ppt] * nb + 7 * (j % ppt);
    pose_col[j] = c0;
    for (int r = 0; r < 7; ++r) col_x[c0 + r] = 7 * j + r;
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
  ba::sim3_pack_values(g->F, g->Z.data(), g->Om.data(), &val);
  constexpr Mem R = Mem::Resident;
  static_assert(sizeof(int4) == 16 && sizeof(int2) == 8, "layout");
  int4 *jk = nullptr;
  int2 *blk = nullptr;
  int32_t *pptr = nullptr, *plist = nullptr, *bptr = nullptr, *blist = nullptr, *opt_pose = nullptr;
  int *pc = nullptr;
  const size_t n7 = (size_t)7 * N;
  if (ba::upload_dense_schedule(h, sc, col_x, g->dd) ||
      h->dalloc(R, &g->Ldiag, (size_t)ncb * ba::dense_ws_per_block(nb)) || h->upload(R, &pc, pose_col) ||
      h->upload(R, &g->zt_I, ztI) || h->upload(R, &g->zt_J, ztJ) ||
      h->upload(R, &d.poses[0], S13, (size_t)g->n_pose * 13) ||
      h->upload(R, &d.poses[1], S13, (size_t)g->n_pose * 13) || h->upload(R, &jk, l.jk.data(), (size_t)g->F) ||
      h->upload(R, &g->val, val) || h->upload(R, &pptr, l.pptr) || h->upload(R, &plist, l.plist) ||
      h->upload(R, &blk, l.blk.data(), l.blk.size() / 2) || h->upload(R, &bptr, l.bptr) ||
      h->upload(R, &blist, l.blist) || h->upload(R, &opt_pose, l.opt_pose) ||
      h->dalloc(R, &d.rec, (size_t)g->F * ba::kS3Rec) || h->dalloc(R, &d.dH, n7) || h->dalloc(R, &d.g, n7) ||
      h->dalloc(R, &d.x, n7 + 64) || h->dalloc(R, &d.part[0], (size_t)d.n_part) ||
      h->dalloc(R, &d.part[1], (size_t)d.n_part) || h->dalloc(R, &d.tpart, (size_t)2 * d.n_tpart) ||
      h->dalloc(R, &g->rep, (size_t)g->F) || h->dalloc(R, &d.ctrl, (size_t)1) ||
      h->dalloc(R, &d.log, (size_t)d.log_cap))
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
  HIP_TRY(hipMemset(d.rec, 0, (size_t)g->F * ba::kS3Rec * sizeof(double)));
  HIP_TRY(hipMemset(d.dH, 0, n7 * sizeof(double)));
  HIP_TRY(hipMemset(d.g, 0, n7 * sizeof(double)));
  HIP_TRY(hipMemset(d.x, 0, (n7 + 64) * sizeof(double)));
  HIP_TRY(hipMemset(d.part[0], 0, (size_t)d.n_part * sizeof(double)));
  HIP_TRY(hipMemset(d.part[1], 0, (size_t)d.n_part * sizeof(double)));
  HIP_TRY(hipMemset(d.tpart, 0, (size_t)2 * d.n_tpart * sizeof(double)));
  HIP_TRY(hipMemset(g->rep, 0, (size_t)g->F * sizeof(double)));
  HIP_TRY(hipMemset(d.ctrl, 0, sizeof(ba::PgCtrl)));
  HIP_TRY(hipEventCreate(&g->e0));
  HIP_TRY(hipEventCreate(&g->e1));
  return 0;
}

// the controller for a pass outside the LM loop: the accepted buffer stays
int begin_pass(ba_sim3 *g) {
  g->hc.done = 0;
  g->hc.relin = 1;
  g->hc.lambda = 0.0;
  return push_ctrl(g);
}

// the device arrays of the robust kernels: kinds 0 and the weights' arrays, once per graph
int ensure_robust_arrays(ba_sim3 *g) {
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
void s3_lin(const ba_sim3 *g, int cost_only, hipStream_t s) {
  if (g->robust)
    ba::launch_s3_lin_robust(g->d, g->rb, cost_only, s);
  else
    ba::launch_s3_lin(g->d, cost_only, nullptr, s);
}
void s3_assemble(const ba_sim3 *g, double *Hout, double *gout, hipStream_t s) {
  if (g->robust)
    ba::launch_s3_assemble_robust(g->d, g->rb, Hout, gout, s);
  else
    ba::launch_s3_assemble(g->d, Hout, gout, s);
}

template <class T>
int download(std::vector<T> &out, const T *dev, size_t n, hipStream_t s) {
  out.resize(n);
  if (n) HIP_TRY(hipMemcpyAsync(out.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
  return 0;
}

// The host arrays of one covariance or gate call (validated): entry_kind = kPgCovPair with
// Z13 = Omega49 = nullptr, or kPgCovCand.  Outputs that are null are not produced.
struct S3CovCall {
  int n_pose_sel = 0;
  const int32_t *pose_sel = nullptr;
  double *cov_pose49 = nullptr;
  int64_t n_entry = 0;
  int entry_kind = ba::kPgCovPair;
  const int32_t *entry_j = nullptr, *entry_k = nullptr;
  const double *Z13 = nullptr, *Omega49 = nullptr;
  double *cov_cross49 = nullptr, *cov_rel49 = nullptr, *d2 = nullptr, *r7 = nullptr, *innov49 = nullptr;
};

// pg_cov_run of ba_pgraph.hip at width 7 (a second driver: the SE(3) one launches its own
// kernels and packs 48-double candidates).  Factorise H at lambda = 0 at the accepted poses with
// the solve's launches, sweep the groups in column batches, copy the blocks out.  The
// controller, the solve's count of dropped pivots and last_ms are as before on return; the
// workspace and the lists are freed on every path.
int s3_cov_run(ba_sim3 *g, const char *what, const S3CovCall &c, int64_t *dropped_pivots) {
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
  s3_lin(g, 0, s);
  ba::launch_dense_init(d.L, d.ld, g->col_x, g->zt_I, g->zt_J, g->n_zt, g->nb, done, s);
  s3_assemble(g, nullptr, nullptr, s);
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
  ba::S3CovOut out{};
  g->cov_batches = 0;
  if (!groups.empty()) {
    std::vector<double> val;
    if (cand) ba::sim3_pack_values(c.n_entry, c.Z13, c.Omega49, &val);
    if (h->upload(R, &d_trow_ptr, trow_ptr) || h->upload(R, &d_trow, trow) || h->upload(R, &d_groups, groups) ||
        h->dalloc(R, &Zw, (size_t)d.npad * bw) || h->dalloc(R, &out.pose49, (size_t)n_pose_rows * 49) ||
        h->dalloc(R, &out.rel49, ne * 49) || (c.cov_cross49 && h->dalloc(R, &out.cross49, ne * 49)) ||
        (cand && (h->upload(R, &d_val, val) || h->dalloc(R, &out.d2, ne))) ||
        (cand && c.r7 && h->dalloc(R, &out.r7, ne * 7)) || (cand && c.innov49 && h->dalloc(R, &out.innov49, ne * 49)))
      return -1;
    for (size_t g0 = 0; g0 < groups.size(); g0 += gpb) {  // fixed batch order
      const int ng = (int)std::min<size_t>(gpb, groups.size() - g0);
      ba::launch_s3cov_batch(d, g->Ldiag, g->nb, g->ncb, d.poses[keep.cur], d_trow_ptr, d_trow, d_groups + g0, ng, d_val,
                             Zw, bw, out, s);
      ++g->cov_batches;
    }
  }
  std::vector<double> hp, hrel, hcross, hd2, hr, hP;
  if (download(hp, out.pose49, (size_t)n_pose_rows * 49, s) || download(hrel, out.rel49, out.rel49 ? ne * 49 : 0, s) ||
      download(hcross, out.cross49, out.cross49 ? ne * 49 : 0, s) || download(hd2, out.d2, out.d2 ? ne : 0, s) ||
      download(hr, out.r7, out.r7 ? ne * 7 : 0, s) || download(hP, out.innov49, out.innov49 ? ne * 49 : 0, s))
    return -1;
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  for (int q = 0; q < c.n_pose_sel; ++q)
    std::memcpy(c.cov_pose49 + (size_t)q * 49, &hp[(size_t)slot_of_opt[g->lists.opt_of_pose[c.pose_sel[q]]] * 49],
                49 * sizeof(double));
  auto give = [](double *dst, const std::vector<double> &src) {
    if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(double));
  };
  if (!cand) give(c.cov_rel49, hrel);
  give(c.cov_cross49, hcross);
  give(c.d2, hd2);
  give(c.r7, hr);
  give(c.innov49, hP);
  if (dropped_pivots) *dropped_pivots = bad_now;
  return 0;
}

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
  HIP_TRY(hipSetDevice(h->device));
  ba_sim3 *g = new ba_sim3();
  g->h = h;
  g->n_pose = n_pose;
  g->F = n_rel;
  if (pose_fixed)
    g->fixed.assign(pose_fixed, pose_fixed + n_pose);
  else
    g->fixed.assign((size_t)n_pose, 0);
  g->Z.assign(Z13, Z13 + 13 * (size_t)n_rel);
  g->Om.assign(Omega49, Omega49 + 49 * (size_t)n_rel);
  ba::pgraph_build_lists(n_pose, g->fixed.data(), n_rel, rel_j, rel_k, &g->lists);
  const size_t mark = h->allocs.size();
  const int rc = build_device(g, S13);
  adopt_allocs(g, mark);
  if (rc) {
    free_graph(g);
    return -1;
  }
  *out = g;
  return 0;
}

void ba_sim3_destroy(ba_sim3 *g) {
  if (!g) return;
  (void)hipSetDevice(g->h->device);
  (void)hipStreamSynchronize(g->h->stream);
  free_graph(g);
}

int ba_sim3_update_values(ba_sim3 *g, const double *S13, const double *Z13, const double *Omega49) {
  if (!g) return fail("ba_sim3_update_values: null graph");
  ba_handle *h = g->h;
  std::string err;
  if (ba::sim3_validate_values(g->n_pose, S13, g->F, Z13, Omega49, &err))
    return fail("ba_sim3_update_values: " + err);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (Z13 || Omega49) {
    if (Z13) g->Z.assign(Z13, Z13 + 13 * (size_t)g->F);
    if (Omega49) g->Om.assign(Omega49, Omega49 + 49 * (size_t)g->F);
    std::vector<double> val;
    ba::sim3_pack_values(g->F, g->Z.data(), g->Om.data(), &val);
    HIP_TRY(hipMemcpy(g->val, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (S13) {
    const size_t bytes = (size_t)g->n_pose * 13 * sizeof(double);
    HIP_TRY(hipMemcpy(g->d.poses[0], S13, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g->d.poses[1], S13, bytes, hipMemcpyHostToDevice));
    g->hc.cur = 0;
  }
  return 0;
}

int ba_sim3_factor_report(ba_sim3 *g, double *s) {
  if (!g || !s) return fail("ba_sim3_factor_report: bad argument");
  ba_handle *h = g->h;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (begin_pass(g)) return -1;
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

int ba_sim3_factor_weights(ba_sim3 *g, double *s, double *w) {
  if (!g) return fail("ba_sim3_factor_weights: null graph");
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
  ba::launch_s3_lin_robust(g->d, rep, 3, h->stream);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  const size_t bytes = (size_t)g->F * sizeof(double);
  if (s) HIP_TRY(hipMemcpy(s, g->d_rep_s, bytes, hipMemcpyDeviceToHost));
  if (w) HIP_TRY(hipMemcpy(w, g->d_rep_w, bytes, hipMemcpyDeviceToHost));
  return 0;
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
  S3CovCall c;
  c.n_pose_sel = n_pose_sel;
  c.pose_sel = pose_sel;
  c.cov_pose49 = cov_pose49;
  c.n_entry = n_pair;
  c.entry_j = pair_j;
  c.entry_k = pair_k;
  c.cov_cross49 = n_pair > 0 ? cov_cross49 : nullptr;
  c.cov_rel49 = cov_rel49;
  return s3_cov_run(g, "ba_sim3_covariance", c, dropped_pivots);
}

int ba_sim3_gate(ba_sim3 *g, int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k, const double *Z13,
                 const double *Omega49, double *d2, double *r7, double *innov49, int64_t *dropped_pivots) {
  if (!g) return fail("ba_sim3_gate: null graph");
  if (ba_sim3_cov_check(g->n_pose, g->fixed.data(), 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, n_cand,
                        cand_j, cand_k, Z13, Omega49, d2))
    return -1;
  S3CovCall c;
  c.n_entry = n_cand;
  c.entry_kind = ba::kPgCovCand;
  c.entry_j = cand_j;
  c.entry_k = cand_k;
  c.Z13 = Z13;
  c.Omega49 = Omega49;
  c.d2 = d2;
  c.r7 = n_cand > 0 ? r7 : nullptr;
  c.innov49 = n_cand > 0 ? innov49 : nullptr;
  return s3_cov_run(g, "ba_sim3_gate", c, dropped_pivots);
}

int ba_sim3_cov_info(ba_sim3 *g, int64_t out4[4]) {
  if (!g || !out4) return fail("ba_sim3_cov_info: bad argument");
  const int bw = ba::cov_batch_cols(g->d.npad, g->h->knobs.run);
  out4[0] = bw;
  out4[1] = ba::kCovGroupCols;
  out4[2] = g->cov_batches;
  out4[3] = (int64_t)g->d.npad * bw * (int64_t)sizeof(double);
  return 0;
}

int ba_sim3_solve(ba_sim3 *g, const ba_options *opt, ba_iter_info *rows, int cap, int *n_iter, int *converged) {
  if (!g || !opt) return fail("ba_sim3_solve: bad argument");
  if (cap < 0 || (cap > 0 && !rows)) return fail("ba_sim3_solve: rows is NULL for cap > 0");
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
    s3_lin(g, 0, s);
    ba::launch_dense_init(d.L, d.ld, g->col_x, g->zt_I, g->zt_J, g->n_zt, g->nb, done, s);
    s3_assemble(g, nullptr, nullptr, s);
    ba::dense_factor_solve(d.L, d.npad, d.ld, g->Ldiag, d.x, done, g->sched, g->dd, g->dd.plan[g->dd.flow_ok], s);
    ba::launch_s3_trial(d, s);
    s3_lin(g, 1, s);
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
  if (bad >= ba::kFlowTimeout) return fail("ba_sim3_solve: a dataflow hand-off timed out");
  g->bad_pivots = bad;
  static_assert(sizeof(ba::DevIterRec) == sizeof(ba_iter_info), "row layout");
  const int n = std::min(std::min(c.iter, cap), d.log_cap);
  if (n > 0) HIP_TRY(hipMemcpy(rows, d.log, (size_t)n * sizeof(ba_iter_info), hipMemcpyDeviceToHost));
  if (n_iter) *n_iter = c.iter;
  if (converged) *converged = c.converged;
  return 0;
}

int ba_sim3_get_poses(ba_sim3 *g, double *S13) {
  if (!g || !S13) return fail("ba_sim3_get_poses: bad argument");
  HIP_TRY(hipSetDevice(g->h->device));
  HIP_TRY(hipStreamSynchronize(g->h->stream));
  HIP_TRY(hipMemcpy(S13, g->d.poses[g->hc.cur], (size_t)g->n_pose * 13 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int ba_sim3_cost(ba_sim3 *g, double *chi2) {
  if (!g || !chi2) return fail("ba_sim3_cost: bad argument");
  HIP_TRY(hipSetDevice(g->h->device));
  if (begin_pass(g)) return -1;
  s3_lin(g, 2, g->h->stream);
  ba::launch_pg_control(g->d, 1, g->h->stream);
  if (pull_ctrl(g)) return -1;
  HIP_TRY(hipGetLastError());
  *chi2 = g->hc.aux;
  return 0;
}

int ba_sim3_get_system(ba_sim3 *g, double *H, double *g7N) {
  if (!g) return fail("ba_sim3_get_system: null graph");
  ba_handle *h = g->h;
  HIP_TRY(hipSetDevice(h->device));
  const size_t n7 = (size_t)7 * g->d.N;
  double *dH = nullptr, *dg = nullptr;
  HIP_TRY(hipMalloc((void **)&dH, n7 * n7 * sizeof(double)));
  if (hipMalloc((void **)&dg, n7 * sizeof(double)) != hipSuccess) {
    (void)hipFree(dH);
    return fail("ba_sim3_get_system: hipMalloc");
  }
  int rc = 0;
  if (hipMemsetAsync(dH, 0, n7 * n7 * sizeof(double), h->stream) != hipSuccess || begin_pass(g)) rc = -1;
  if (!rc) {
    s3_lin(g, 0, h->stream);
    s3_assemble(g, dH, dg, h->stream);
    if (hipStreamSynchronize(h->stream) != hipSuccess || hipGetLastError() != hipSuccess ||
        (H && hipMemcpy(H, dH, n7 * n7 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
        (g7N && hipMemcpy(g7N, dg, n7 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
      rc = fail("ba_sim3_get_system: device error");
  }
  (void)hipFree(dH);
  (void)hipFree(dg);
  return rc;
}

int ba_sim3_info(ba_sim3 *g, int64_t out9[9]) {
  if (!g || !out9) return fail("ba_sim3_info: bad argument");
  out9[0] = g->d.N;
  out9[1] = g->F;
  out9[2] = g->d.nblk;
  out9[3] = g->nb;
  out9[4] = g->ncb;
  out9[5] = g->sched.nlev;
  out9[6] = (int64_t)g->image_bytes;
  out9[7] = g->bad_pivots;
  out9[8] = ba::kS3Fpb;
  return 0;
}

int ba_sim3_last_ms(ba_sim3 *g, double *ms) {
  if (!g || !ms) return fail("ba_sim3_last_ms: bad argument");
  *ms = g->last_ms;
  return 0;
}

}  // extern "C"
