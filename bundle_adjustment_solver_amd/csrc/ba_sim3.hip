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
// The host side is the graph driver of ba_graph.hip, which this graph shares with the SE(3) one
// (ba_pgraph.hip): below the kernels this file has the driver's description of a Sim(3) graph
// (kS3Spec: the widths, these launchers) and the ba_sim3_* entry points, which validate and call
// the driver.  Covariance blocks and the gate (ba_sim3_covariance / ba_sim3_gate):
// the driver's graph_cov_run (the solve's launches at lambda = 0, then column batches), the groups
// are the pose graph's (ba_pgraph_host.h), the validation in ba_sim3_host.h, the kernels in
// ba_sim3_cov.hip.
#include <type_traits>

#include "ba_graph.h"
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
// The driver is ba_graph.hip; here are the Sim(3) graph's spec and its entry points, which check
// their pointers, validate the caller's arrays and call the driver.  ba_sim3_factor_report alone
// launches a kernel itself: the plain k_s3_lin with an array for s_f.
using ba::fail;

struct ba_sim3 : ba::GraphHost {
  double *rep = nullptr;  // s_f per factor of ba_sim3_factor_report (allocated by its first call)
};

namespace {

void s3_lin(const ba::PgDev &p, int cost_only, hipStream_t s) { ba::launch_s3_lin(p, cost_only, nullptr, s); }

void s3_cov_batch(const ba::PgDev &p, const double *Ldiag, int nb, int ncb, const double *poses, const int *trow_ptr,
                  const int *trow, const ba::PgCovGroup *groups, int ng, const double *cand_val, double *Zw, int bw,
                  const ba::GraphCovOut &o, hipStream_t s) {
  const ba::S3CovOut out{o.pose, o.cross, o.rel, o.r, o.innov, o.d2};
  ba::launch_s3cov_batch(p, Ldiag, nb, ncb, poses, trow_ptr, trow, groups, ng, cand_val, Zw, bw, out, s);
}

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
    s3_lin,
    ba::launch_s3_lin_robust,
    ba::launch_s3_assemble,
    ba::launch_s3_assemble_robust,
    ba::launch_s3_trial,
    s3_cov_batch,
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
