// ba_batch.hip — batched full bundle adjustment: B independent small problems (sliding
// windows), ONE persistent 256-thread workgroup each, the whole LM loop of
// FullBundleAdjustmentSolver::Solve (reference core/full_bundle_adjustment_solver.cpp:
// 705-1008) in one launch.  No grid barrier and no workgroup waits on another: a batch
// larger than the device holds at once drains.  The arithmetic is the handle path's
// (ba_device_fn.h, ba_chol_lds.h); the sums are ordered per problem only, so a problem
// gives the same bits alone and at any position of any batch.
//
// Per iteration of one workgroup (fp64 throughout):
//   landmark pass   one thread per optimisable landmark, its observations in insertion
//                   order: C_i, b_i, and B_ji of the LAST observation of a (landmark, pose)
//                   pair (reference :826)                               -> global scratch
//   pose pass       one wave per optimisable pose, its observations strided over the
//                   lanes, 27 wave sums: A_j, a_j                        -> LDS
//                   (both passes are skipped after a SKIPPED step: the blocks are stored
//                   undamped and are still the linearisation at the accepted point)
//   damp / invert   C_i (1 + lambda) -> Cinv_i, Cinv_i b_i              -> global scratch
//   Schur           one thread per half 6x6 block (3 rows) of the lower triangle of S, the
//                   landmarks in ascending order through the (landmark, pose) -> pair table;
//                   rhs_j = a_j - sum_i B_ji Cinv_i b_i                  -> LDS image
//   reduced solve   chol_lds_factor_solve on the LDS image (<= 96 columns + rhs block)
//   back-substitution, trial point, quadratic model, step norms; trial cost; control step
//
// k_ba_batch_cov (ba_batch_covariance) reuses the first half — the two linearisation passes,
// damp / invert with lambda = 0, Schur and the factorisation, shared as device functions —
// and then inverts the factor in LDS (chol_lds_inverse) and reads the covariance blocks of
// every pose and landmark of the problem off S^-1.
//
// k_ba_batch_marg (ba_batch_marginalize) runs the same first half over the landmarks the
// marked poses observe only, with the marked poses' columns first in the image, and stops
// the factorisation after them (chol_lds_partial): the trailing update is the prior the
// window leaves on its kept poses.
//
// A pose prior per problem (ba_batch_set_prior): the Gaussian 1/2 d^T H d - b^T d + c / 2 on
// K of its optimisable poses, d_j = se3_log(T_j T_lin,j^-1), is one more factor of all three
// kernels (batch_prior_lin / batch_prior_offdiag / batch_prior_cost).  H stays in
// global memory; the branch is uniform per workgroup and a problem without a prior executes
// none of it.
//
// Relative-pose factors per problem (ba_batch_set_relative): r = se3_log(T_j T_k^-1 Z^-1)
// against a measurement Z of T_j T_k^-1 with a 6x6 information matrix, Jacobians of first order
// (I and -Ad(T_j T_k^-1)), no robust weight; the factor is defined once for all three paths, on
// the device in ba_rel_fn.h and on the host in ba_rel_host.h.  Their blocks depend on the poses and are rebuilt
// per linearisation into global scratch (batch_rel_lin / batch_rel_offdiag / batch_rel_cross /
// batch_rel_cost); nothing per factor lives in LDS.  Each kernel exists with and without that
// code; this file compiles the instances without, which a batch without factors launches, and
// ba_batch_rel.hip the others.  The device side of both is ba_batch_kernels.h.
//
// Host side: ba_batch_create plans the structure once (stable landmark-major grouping,
// pair lists, last-writer marks, one upload); ba_batch_solve is one launch and one sync.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ba_batch_kernels.h"
#include "ba_batch_obs.h"
#include "ba_batch_obs_host.h"
#include "ba_rel_host.h"

// ===========================================================================================
// host side
// ===========================================================================================
using ba::fail;

struct ba_batch {
  ba_handle *h = nullptr;  // borrowed (device and stream): the handle outlives the batch
  int B = 0;
  int npt_class = 6;  // 16-column panels of the LDS image: 2, 4 or 6
  int max_N = 0;
  std::vector<ba::BatchProb> prob;
  int64_t n_cam = 0, n_pose = 0, n_pt = 0, n_obs = 0, n_pair = 0, n_m = 0;
  int64_t max_scratch = 0;
  char *dev = nullptr;  // one allocation: structure | parameters | scratch
  size_t dev_bytes = 0;
  ba::BatchDev d{};
  ba::DevIterRec *rows = nullptr;
  size_t rows_cap = 0;  // records
  char *cov = nullptr;  // outputs of ba_batch_covariance (allocated by its first call)
  size_t cov_bytes = 0, cov_pt_off = 0, cov_res_off = 0;
  std::vector<int32_t> jopt;  // per pose of the batch: optimisable index or -1 (host copy)
  char *marg = nullptr;       // inputs and outputs of ba_batch_marginalize (grown on demand)
  size_t marg_bytes = 0;
  char *prior = nullptr;  // the pose priors (ba_batch_set_prior): records | poses | T_lin | H | b
  size_t prior_bytes = 0;
  int64_t prior_n = 0, prior_K = 0;  // problems with a prior in effect, their poses
  char *rel = nullptr;  // the relative-pose factors (ba_batch_set_relative): records | lists | scratch
  size_t rel_bytes = 0;
  int64_t rel_n = 0, rel_F = 0;  // problems with factors in effect, their factors
  const ba::BatchRelDev *relp = nullptr;  // device record of their arrays, the argument of the REL instances
  std::vector<int32_t> rel_off, rel_j, rel_k;  // the factors as given (ba_batch_relative_marg_plan)
  // the observation mask (ba_batch_set_obs_mask, ba_batch_cull): allocated by the first call that needs it
  std::vector<int32_t> order;  // per planned observation: its user index (problem-local)
  char *mask = nullptr;        // order | flags | shadow lists | cull results | first-stage results
  size_t mask_bytes = 0;
  bool masked = false;         // d points at the shadow lists
  ba::BatchMaskDev md{};
  ba_batch_result *res_first = nullptr;  // device, B records (ba_batch_solve_culled)
  ba::BatchDev lists0{};       // d as ba_batch_create left it: the planned lists
  char *rep = nullptr;         // outputs of ba_batch_obs_report (allocated by its first call)
};

namespace {

// Structure of ONE problem (host only): the stable landmark-major order of its
// observations, the (landmark, pose) pairs of optimisable members in (landmark, pose)
// order, and per observation its pair and whether it is the pair's last writer.
struct ProbPlan {
  std::vector<int32_t> jopt, iopt, opt_lm, order, lm_ptr, pair_ptr, pair_j, obs_pair, tab, pobs, pobs_ptr;
  std::vector<uint8_t> last;
  int N = 0, M = 0;
};

// device scratch of one problem: C, b, Cinv, Cinv*b of its M landmarks (6+3+6+3 doubles),
// W of its P pairs (18) and its trial points (3 each)
int64_t scratch_bytes_of(const ba::BatchProb &P) {
  return (int64_t)sizeof(double) * ((int64_t)P.M * 18 + (int64_t)P.P * 18 + (int64_t)P.n_pt * 3);
}

void plan_problem(int n_pose, const uint8_t *pose_fixed, int n_pt, const uint8_t *pt_fixed, int64_t n_obs,
                  const int32_t *obs_pose, const int32_t *obs_pt, ProbPlan &pl) {
  pl.jopt.assign(n_pose, -1);
  pl.iopt.assign(n_pt, -1);
  pl.N = pl.M = 0;
  for (int p = 0; p < n_pose; ++p)
    if (!(pose_fixed && pose_fixed[p])) pl.jopt[p] = pl.N++;
  pl.opt_lm.clear();
  for (int q = 0; q < n_pt; ++q)
    if (!(pt_fixed && pt_fixed[q])) {
      pl.iopt[q] = pl.M++;
      pl.opt_lm.push_back(q);
    }
  pl.order.resize(n_obs);
  for (int64_t k = 0; k < n_obs; ++k) pl.order[k] = (int32_t)k;
  std::stable_sort(pl.order.begin(), pl.order.end(),
                   [&](int32_t a, int32_t b) { return obs_pt[a] < obs_pt[b]; });
  pl.lm_ptr.assign(n_pt + 1, 0);
  for (int64_t k = 0; k < n_obs; ++k) pl.lm_ptr[obs_pt[k] + 1]++;
  for (int q = 0; q < n_pt; ++q) pl.lm_ptr[q + 1] += pl.lm_ptr[q];
  pl.pair_ptr.assign(pl.M + 1, 0);
  pl.pair_j.clear();
  pl.tab.assign((size_t)pl.M * pl.N, -1);
  pl.obs_pair.assign(n_obs, -1);
  pl.last.assign(n_obs, 0);
  std::vector<int32_t> js;
  for (int i = 0; i < pl.M; ++i) {
    const int q = pl.opt_lm[i];
    js.clear();
    for (int t = pl.lm_ptr[q]; t < pl.lm_ptr[q + 1]; ++t) {
      const int j = pl.jopt[obs_pose[pl.order[t]]];
      if (j >= 0) js.push_back(j);
    }
    std::sort(js.begin(), js.end());
    js.erase(std::unique(js.begin(), js.end()), js.end());
    for (int32_t j : js) {
      pl.tab[(size_t)i * pl.N + j] = (int32_t)pl.pair_j.size();
      pl.pair_j.push_back(j);
    }
    pl.pair_ptr[i + 1] = (int32_t)pl.pair_j.size();
    // the last observation (insertion order) of each pair is its writer (reference :826)
    for (int t = pl.lm_ptr[q + 1] - 1; t >= pl.lm_ptr[q]; --t) {
      const int j = pl.jopt[obs_pose[pl.order[t]]];
      if (j < 0) continue;
      const int32_t pid = pl.tab[(size_t)i * pl.N + j];
      pl.obs_pair[t] = pid;
      bool later = false;
      for (int t2 = t + 1; t2 < pl.lm_ptr[q + 1] && !later; ++t2)
        later = pl.obs_pair[t2] == pid;
      pl.last[t] = later ? 0 : 1;
    }
  }
  // pose-major index of the landmark-major list
  pl.pobs_ptr.assign(pl.N + 1, 0);
  for (int64_t t = 0; t < n_obs; ++t) {
    const int j = pl.jopt[obs_pose[pl.order[t]]];
    if (j >= 0) pl.pobs_ptr[j + 1]++;
  }
  for (int j = 0; j < pl.N; ++j) pl.pobs_ptr[j + 1] += pl.pobs_ptr[j];
  pl.pobs.resize(pl.pobs_ptr[pl.N]);
  std::vector<int32_t> fill(pl.pobs_ptr.begin(), pl.pobs_ptr.end() - 1);
  for (int64_t t = 0; t < n_obs; ++t) {
    const int j = pl.jopt[obs_pose[pl.order[t]]];
    if (j >= 0) pl.pobs[fill[j]++] = (int32_t)t;
  }
}

template <class T>
size_t put(std::vector<char> &blob, const std::vector<T> &v) {
  size_t o = (blob.size() + 255) & ~(size_t)255;
  blob.resize(o + v.size() * sizeof(T));
  if (!v.empty()) std::memcpy(blob.data() + o, v.data(), v.size() * sizeof(T));
  return o;
}

int batch_check_offsets(const char *name, int B, const int64_t *off, bool strict) {
  if (!off) return fail(std::string("ba_batch_create: null ") + name);
  if (off[0] != 0) return fail(std::string("ba_batch_create: ") + name + "[0] must be 0");
  for (int b = 0; b < B; ++b)
    if (off[b + 1] < off[b] || (strict && off[b + 1] == off[b]))
      return fail(std::string("ba_batch_create: ") + name + " must " + (strict ? "increase" : "not decrease") +
                  " (problem " + std::to_string(b) + ")");
  return 0;
}

// the host's plan of every problem for one marking, and the 16-column panels of the widest
// image among the problems that will be processed
int marg_plan_batch(const ba_batch *b, const uint8_t *marg_pose, std::vector<ba::BatchMargProb> &mp) {
  mp.resize(b->B);
  int64_t ho = 0, bo = 0;
  int tiles = 1;
  for (int p = 0; p < b->B; ++p) {
    const ba::BatchProb &P = b->prob[p];
    int K = 0, m = 0;
    for (int q = 0; q < P.n_pose; ++q)
      if (b->jopt[P.pose0 + q] >= 0) (marg_pose[P.pose0 + q] ? m : K)++;
    mp[p] = ba::BatchMargProb{ho, bo, K, m};
    ho += (int64_t)36 * K * K;
    bo += (int64_t)6 * K;
    if (P.status == 0) tiles = std::max(tiles, (16 * ((6 * m + 15) / 16) + 6 * K + 15) / 16);
  }
  return tiles;
}

// Validation shared by ba_batch_set_prior and ba_batch_prior_check (host only).  n_pose_of(p)
// and fixed(p, q) describe the batch; who prefixes the message.
template <class NP, class FX>
int prior_validate(const char *who, int B, NP n_pose_of, FX fixed, const int32_t *prior_off,
                   const int32_t *prior_pose, const double *T_lin12, const double *H, const double *bvec,
                   const double *c) {
  const std::string w = std::string(who) + ": ";
  if (!prior_off) return fail(w + "null prior_off");
  if (prior_off[0] != 0) return fail(w + "prior_off[0] must be 0");
  for (int p = 0; p < B; ++p)
    if (prior_off[p + 1] < prior_off[p])
      return fail(w + "prior_off must not decrease (problem " + std::to_string(p) + ")");
  if (prior_off[B] > 0 && (!prior_pose || !T_lin12 || !H || !bvec)) return fail(w + "null prior array");
  int64_t ho = 0;
  for (int p = 0; p < B; ++p) {
    const int k0 = prior_off[p], K = prior_off[p + 1] - k0;
    const std::string at = " (problem " + std::to_string(p) + ")";
    for (int t = 0; t < K; ++t) {
      const int q = prior_pose[k0 + t];
      if (q < 0 || q >= n_pose_of(p)) return fail(w + "prior pose " + std::to_string(q) + " out of range" + at);
      if (t > 0 && q <= prior_pose[k0 + t - 1]) return fail(w + "prior poses must ascend strictly" + at);
      if (fixed(p, q)) return fail(w + "prior pose " + std::to_string(q) + " is fixed" + at);
    }
    for (int64_t e = 0; e < (int64_t)12 * K; ++e)
      if (!std::isfinite(T_lin12[(int64_t)12 * k0 + e])) return fail(w + "T_lin is not finite" + at);
    for (int64_t e = 0; e < (int64_t)36 * K * K; ++e)
      if (!std::isfinite(H[ho + e])) return fail(w + "H is not finite" + at);
    for (int64_t e = 0; e < (int64_t)6 * K; ++e)
      if (!std::isfinite(bvec[(int64_t)6 * k0 + e])) return fail(w + "b is not finite" + at);
    if (c && !(std::isfinite(c[p]) && c[p] >= 0.0)) return fail(w + "c must be finite and >= 0" + at);
    ho += (int64_t)36 * K * K;
  }
  return 0;
}

// Validation shared by ba_batch_set_relative and ba_batch_relative_check (host only).
template <class NP, class FX>
int relative_validate(const char *who, int B, NP n_pose_of, FX fixed, const int32_t *rel_off, const int32_t *rel_j,
                      const int32_t *rel_k, const double *Z12, const double *Omega36) {
  const std::string w = std::string(who) + ": ";
  if (!rel_off) return fail(w + "null rel_off");
  if (rel_off[0] != 0) return fail(w + "rel_off[0] must be 0 (problem 0)");
  for (int p = 0; p < B; ++p)
    if (rel_off[p + 1] < rel_off[p]) return fail(w + "rel_off must not decrease (problem " + std::to_string(p) + ")");
  // the rules of a factor are relative_validate_host's, per problem with factors (the first reports a null array)
  std::vector<uint8_t> fx;
  std::string err;
  for (int p = 0; p < B; ++p) {
    const int64_t f0 = rel_off[p];
    if (rel_off[p + 1] == f0) continue;
    const int np = n_pose_of(p);
    fx.resize((size_t)np);
    for (int q = 0; q < np; ++q) fx[q] = fixed(p, q) ? 1 : 0;
    auto at = [f0](const auto *a, int per) { return a ? a + per * f0 : a; };
    const int what = ba::kRelPairs | ba::kRelValues | ba::kRelNoPoseOk;
    if (ba::relative_validate_host(what, np, fx.data(), rel_off[p + 1] - f0, at(rel_j, 1), at(rel_k, 1), at(Z12, 12),
                                   at(Omega36, 36), &err, "problem " + std::to_string(p) + ", "))
      return fail(w + err);
  }
  return 0;
}

void relative_drop(ba_batch *b) {
  if (b->rel) (void)hipFree(b->rel);
  b->rel = nullptr;
  b->rel_bytes = 0;
  b->rel_n = b->rel_F = 0;
  b->rel_off.clear();
  b->rel_j.clear();
  b->rel_k.clear();
  b->relp = nullptr;
}

size_t lds_bytes_of(int npt) {
  return npt == 2 ? sizeof(ba::BatchLds<2>) : npt == 4 ? sizeof(ba::BatchLds<4>) : sizeof(ba::BatchLds<6>);
}

// the device rows of a solve: room for n_rows records
int rows_reserve(ba_batch *b, size_t n_rows) {
  if (n_rows > b->rows_cap) {
    if (b->rows) (void)hipFree(b->rows);
    b->rows = nullptr;
    b->rows_cap = 0;
    HIP_TRY(hipMalloc((void **)&b->rows, n_rows * sizeof(ba::DevIterRec)));
    b->rows_cap = n_rows;
  }
  return 0;
}

// one solve of the batch on the handle's stream: d carries the lists, rows, cap and res of the
// launch, the options are promoted here
void solve_launch(ba_batch *b, const ba_options *opt, ba::BatchDev &d) {
  hipStream_t s = b->h->stream;
  const int B = b->B;
  d.lambda0 = (double)opt->initial_lambda;
  d.huber = (double)opt->threshold_huber_loss;
  d.thr_step = (double)opt->threshold_step_size;
  d.thr_cost = (double)opt->threshold_cost_change;
  d.dec_ratio = (double)opt->decrease_ratio_lambda;
  d.inc_ratio = (double)opt->increase_ratio_lambda;
  d.max_iter = opt->max_num_iterations;
  d.gn = opt->gauss_newton ? 1 : 0;
  if (b->relp)  // the instances with the factor code, and their arrays, only for a batch that has factors
    ba::batch_launch_rel(0, b->npt_class, B, s, &d, nullptr, b->relp);
  else if (b->npt_class == 2)
    hipLaunchKernelGGL((ba::k_ba_batch<2, false>), dim3(B), dim3(ba::kBatchBlock), 0, s, d);
  else if (b->npt_class == 4)
    hipLaunchKernelGGL((ba::k_ba_batch<4, false>), dim3(B), dim3(ba::kBatchBlock), 0, s, d);
  else
    hipLaunchKernelGGL((ba::k_ba_batch<6, false>), dim3(B), dim3(ba::kBatchBlock), 0, s, d);
}

// which lists the kernels read: the planned ones, or their shadows without the off observations
void mask_point(ba_batch *b, bool shadow) {
  const ba::BatchMaskDev &m = b->md;
  b->d.prob = shadow ? m.prob_s : b->lists0.prob;
  b->d.lobs = shadow ? m.lobs_s : b->lists0.lobs;
  b->d.luv = shadow ? m.luv_s : b->lists0.luv;
  b->d.lm_ptr = shadow ? m.lm_ptr_s : b->lists0.lm_ptr;
  b->d.pobs = shadow ? m.pobs_s : b->lists0.pobs;
  b->d.pobs_ptr = shadow ? m.pobs_ptr_s : b->lists0.pobs_ptr;
  b->masked = shadow;
}

// the device side of the mask, allocated once: the permutation uploaded, every flag on
int mask_ensure(ba_batch *b) {
  if (b->mask) return 0;
  const size_t nobs = (size_t)b->n_obs, B = (size_t)b->B;
  const size_t n_pptr = (size_t)b->prob.back().pptr0 + b->prob.back().N + 1;
  const size_t n_po = nobs;  // the pose-major list holds the observations of optimisable poses: never more
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t o = 0;
  const size_t o_ord = o;   o = al(o + nobs * sizeof(int32_t));
  const size_t o_on = o;    o = al(o + nobs);
  const size_t o_try = o;   o = al(o + nobs);
  const size_t o_pre = o;   o = al(o + (nobs + B) * sizeof(int32_t));
  const size_t o_lobs = o;  o = al(o + nobs * sizeof(int4));
  const size_t o_luv = o;   o = al(o + nobs * sizeof(double2));
  const size_t o_lm = o;    o = al(o + ((size_t)b->n_pt + B) * sizeof(int32_t));
  const size_t o_po = o;    o = al(o + n_po * sizeof(int32_t));
  const size_t o_pp = o;    o = al(o + n_pptr * sizeof(int32_t));
  const size_t o_prob = o;  o = al(o + B * sizeof(ba::BatchProb));
  const size_t o_cres = o;  o = al(o + B * sizeof(ba_batch_cull_result));
  const size_t o_res1 = o;  o = al(o + B * sizeof(ba_batch_result));
  char *M = nullptr;
  if (hipMalloc((void **)&M, o) != hipSuccess)
    return fail("ba_batch: device allocation of " + std::to_string(o) + " bytes for the observation mask failed");
  hipStream_t s = b->h->stream;
  if (hipMemsetAsync(M, 0, o, s) != hipSuccess || hipMemsetAsync(M + o_on, 1, nobs, s) != hipSuccess ||
      (nobs && hipMemcpyAsync(M + o_ord, b->order.data(), nobs * sizeof(int32_t), hipMemcpyHostToDevice, s) !=
                   hipSuccess) ||
      hipStreamSynchronize(s) != hipSuccess) {
    (void)hipFree(M);
    return fail("ba_batch: upload of the observation order failed");
  }
  b->mask = M;
  b->mask_bytes = o;
  ba::BatchMaskDev &m = b->md;
  const ba::BatchDev &l = b->lists0;
  m.prob = l.prob;
  m.cams = l.cams;
  m.poses = l.poses;
  m.pts = l.pts[0];
  m.jopt = l.jopt;
  m.opt_lm = l.opt_lm;
  m.order = (const int32_t *)(M + o_ord);
  m.lobs = l.lobs;
  m.luv = l.luv;
  m.lm_ptr = l.lm_ptr;
  m.pair_ptr = l.pair_ptr;
  m.pobs = l.pobs;
  m.pobs_ptr = l.pobs_ptr;
  m.on = (uint8_t *)(M + o_on);
  m.on_try = (uint8_t *)(M + o_try);
  m.pre = (int32_t *)(M + o_pre);
  m.lobs_s = (int4 *)(M + o_lobs);
  m.luv_s = (double2 *)(M + o_luv);
  m.lm_ptr_s = (int32_t *)(M + o_lm);
  m.pobs_s = (int32_t *)(M + o_po);
  m.pobs_ptr_s = (int32_t *)(M + o_pp);
  m.prob_s = (ba::BatchProb *)(M + o_prob);
  m.W18 = l.W18;
  m.cres = (ba_batch_cull_result *)(M + o_cres);
  b->res_first = (ba_batch_result *)(M + o_res1);
  return 0;
}

void mask_apply_launch(ba_batch *b) {
  hipLaunchKernelGGL(ba::k_ba_batch_mask_apply, dim3(b->B), dim3(ba::kBatchBlock), 0, b->h->stream, b->md);
  mask_point(b, true);
}

void cull_launch(ba_batch *b, const ba_cull_options *c) {
  hipLaunchKernelGGL(ba::k_ba_batch_cull, dim3(b->B), dim3(ba::kBatchBlock), 0, b->h->stream, b->md, c->e2_max,
                     c->cull_behind ? 1 : 0);
  mask_apply_launch(b);
}

int cull_refuse(const char *who, const ba_batch *b, const ba_cull_options *c, const ba_batch_cull_result *cres) {
  const std::string w = std::string(who) + ": ";
  if (!b) return fail(w + "null batch");
  std::string err;
  if (ba::cull_validate_host(c ? &c->e2_max : nullptr, &err)) return fail(w + err);
  if (!cres) return fail(w + "null cres");
  return 0;
}

}  // namespace

extern "C" {

int ba_batch_plan_problem(int n_pose, const uint8_t *pose_fixed, int n_pt, const uint8_t *pt_fixed, int64_t n_obs,
                          const int32_t *obs_pose, const int32_t *obs_pt, int32_t *order, int32_t *obs_pair,
                          uint8_t *last_writer, int32_t *pair_lm, int32_t *pair_pose) {
  if (n_pose < 0 || n_pt < 0 || n_obs < 0 || n_obs > INT32_MAX) return fail("ba_batch_plan_problem: bad sizes");
  if (n_obs > 0 && (!obs_pose || !obs_pt)) return fail("ba_batch_plan_problem: null observations");
  for (int64_t k = 0; k < n_obs; ++k)
    if (obs_pose[k] < 0 || obs_pose[k] >= n_pose || obs_pt[k] < 0 || obs_pt[k] >= n_pt)
      return fail("ba_batch_plan_problem: observation " + std::to_string(k) + " out of range");
  ProbPlan pl;
  plan_problem(n_pose, pose_fixed, n_pt, pt_fixed, n_obs, obs_pose, obs_pt, pl);
  for (int64_t t = 0; t < n_obs; ++t) {
    if (order) order[t] = pl.order[t];
    if (obs_pair) obs_pair[t] = pl.obs_pair[t];
    if (last_writer) last_writer[t] = pl.last[t];
  }
  for (int i = 0; i < pl.M; ++i)
    for (int p = pl.pair_ptr[i]; p < pl.pair_ptr[i + 1]; ++p) {
      if (pair_lm) pair_lm[p] = i;
      if (pair_pose) pair_pose[p] = pl.pair_j[p];
    }
  return (int)pl.pair_j.size();
}

int ba_batch_create(ba_batch **out, ba_handle *h, int B, const int32_t *cam_off, const int32_t *pose_off,
                    const int32_t *pt_off, const int64_t *obs_off, const double *cam_intr4, const double *cam_T12,
                    const double *pose_T12, const uint8_t *pose_fixed, const double *pt_X3, const uint8_t *pt_fixed,
                    const int32_t *obs_cam, const int32_t *obs_pose, const int32_t *obs_pt, const double *obs_uv2) {
  if (out) *out = nullptr;
  if (!out) return fail("ba_batch_create: null out");
  if (B < 1) return fail("ba_batch_create: B must be >= 1");
  if (!cam_off || !pose_off || !pt_off || !obs_off) return fail("ba_batch_create: null offsets");
  {
    std::vector<int64_t> t(B + 1);
    const int32_t *o32[3] = {cam_off, pose_off, pt_off};
    const char *nm[3] = {"cam_off", "pose_off", "pt_off"};
    for (int a = 0; a < 3; ++a) {
      for (int b = 0; b <= B; ++b) t[b] = o32[a][b];
      if (batch_check_offsets(nm[a], B, t.data(), false)) return -1;
    }
    if (batch_check_offsets("obs_off", B, obs_off, false)) return -1;
  }
  if (!cam_intr4 || !cam_T12 || !pose_T12 || !pt_X3) return fail("ba_batch_create: null parameter array");
  if (obs_off[B] > 0 && (!obs_cam || !obs_pose || !obs_pt || !obs_uv2))
    return fail("ba_batch_create: null observation array");
  for (int b = 0; b < B; ++b) {
    const int nc = cam_off[b + 1] - cam_off[b], np = pose_off[b + 1] - pose_off[b], nq = pt_off[b + 1] - pt_off[b];
    if (obs_off[b + 1] - obs_off[b] > INT32_MAX)
      return fail("ba_batch_create: problem " + std::to_string(b) + " has too many observations");
    for (int64_t k = obs_off[b]; k < obs_off[b + 1]; ++k)
      if (obs_cam[k] < 0 || obs_cam[k] >= nc || obs_pose[k] < 0 || obs_pose[k] >= np || obs_pt[k] < 0 ||
          obs_pt[k] >= nq)
        return fail("ba_batch_create: observation " + std::to_string(k - obs_off[b]) + " of problem " +
                    std::to_string(b) + " has an index outside its problem");
  }
  if (!h) return fail("ba_batch_create: null handle");
  if (h->world > 1 || h->ar_fn) return fail("ba_batch_create: a sharded handle cannot run a batch");
  if (h->arena) return fail("ba_batch_create: a streamed handle cannot run a batch");

  ba_batch *bt = new ba_batch();
  bt->h = h;
  bt->B = B;
  bt->prob.resize(B);
  bt->n_cam = cam_off[B];
  bt->n_pose = pose_off[B];
  bt->n_pt = pt_off[B];
  bt->n_obs = obs_off[B];
  std::vector<double> cams((size_t)bt->n_cam * 16);
  for (int64_t c = 0; c < bt->n_cam; ++c) {
    std::memcpy(&cams[c * 16], cam_intr4 + 4 * c, 4 * sizeof(double));
    std::memcpy(&cams[c * 16 + 4], cam_T12 + 12 * c, 12 * sizeof(double));
  }
  std::vector<int32_t> jopt(bt->n_pose), opt_lm, lm_ptr, pair_ptr, pair_j, tab, pobs, pobs_ptr;
  std::vector<int4> lobs(bt->n_obs);
  std::vector<double2> luv(bt->n_obs);
  lm_ptr.reserve(bt->n_pt + B);
  ProbPlan pl;
  for (int b = 0; b < B; ++b) {
    ba::BatchProb &P = bt->prob[b];
    P.n_cam = cam_off[b + 1] - cam_off[b];
    P.n_pose = pose_off[b + 1] - pose_off[b];
    P.n_pt = pt_off[b + 1] - pt_off[b];
    P.n_obs = (int32_t)(obs_off[b + 1] - obs_off[b]);
    P.cam0 = cam_off[b];
    P.pose0 = pose_off[b];
    P.pt0 = pt_off[b];
    P.obs0 = obs_off[b];
    plan_problem(P.n_pose, pose_fixed ? pose_fixed + P.pose0 : nullptr, P.n_pt, pt_fixed ? pt_fixed + P.pt0 : nullptr,
                 P.n_obs, obs_pose + P.obs0, obs_pt + P.obs0, pl);
    P.N = pl.N;
    P.M = pl.M;
    P.P = (int32_t)pl.pair_j.size();
    P.status = (P.N > ba::kBatchMaxOpt || P.n_pose > ba::kBatchMaxPoses || P.n_cam > ba::kCamLds) ? 2 : 0;
    P.pair0 = (int64_t)pair_j.size();
    P.m0 = (int64_t)opt_lm.size();
    P.tab0 = (int64_t)tab.size();
    P.pobs0 = (int64_t)pobs.size();
    P.pptr0 = (int64_t)pobs_ptr.size();
    for (int p = 0; p < P.n_pose; ++p) jopt[P.pose0 + p] = pl.jopt[p];
    bt->order.insert(bt->order.end(), pl.order.begin(), pl.order.end());
    for (int t = 0; t < P.n_obs; ++t) {
      const int64_t k = P.obs0 + pl.order[t];
      const int32_t pid = pl.obs_pair[t];
      lobs[P.obs0 + t] = make_int4(obs_cam[k], obs_pose[k], obs_pt[k], pid < 0 ? -1 : (pid << 1 | pl.last[t]));
      luv[P.obs0 + t] = make_double2(obs_uv2[2 * k], obs_uv2[2 * k + 1]);
    }
    opt_lm.insert(opt_lm.end(), pl.opt_lm.begin(), pl.opt_lm.end());
    lm_ptr.insert(lm_ptr.end(), pl.lm_ptr.begin(), pl.lm_ptr.end());      // at pt0 + b
    pair_ptr.insert(pair_ptr.end(), pl.pair_ptr.begin(), pl.pair_ptr.end());  // at m0 + b
    pair_j.insert(pair_j.end(), pl.pair_j.begin(), pl.pair_j.end());
    tab.insert(tab.end(), pl.tab.begin(), pl.tab.end());
    pobs.insert(pobs.end(), pl.pobs.begin(), pl.pobs.end());
    pobs_ptr.insert(pobs_ptr.end(), pl.pobs_ptr.begin(), pl.pobs_ptr.end());
    if (P.status == 0) bt->max_N = std::max(bt->max_N, P.N);
    bt->max_scratch = std::max(bt->max_scratch, scratch_bytes_of(P));
  }
  bt->n_pair = (int64_t)pair_j.size();
  bt->n_m = (int64_t)opt_lm.size();
  bt->jopt = jopt;
  bt->npt_class = bt->max_N <= 5 ? 2 : bt->max_N <= 10 ? 4 : 6;

  // one host image, one upload: structure | parameters; the scratch follows it on the device
  std::vector<char> blob;
  std::vector<double> poses(pose_T12, pose_T12 + (size_t)bt->n_pose * 12), pts(pt_X3, pt_X3 + (size_t)bt->n_pt * 3);
  const size_t o_prob = put(blob, bt->prob), o_cams = put(blob, cams), o_jopt = put(blob, jopt),
               o_optlm = put(blob, opt_lm), o_lobs = put(blob, lobs), o_luv = put(blob, luv),
               o_lmptr = put(blob, lm_ptr), o_pptr = put(blob, pair_ptr), o_pj = put(blob, pair_j),
               o_tab = put(blob, tab), o_pobs = put(blob, pobs), o_poptr = put(blob, pobs_ptr),
               o_poses = put(blob, poses), o_pts = put(blob, pts);
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t o = al(blob.size());
  const size_t o_pts1 = o;  o = al(o + (size_t)bt->n_pt * 3 * sizeof(double));
  const size_t o_C = o;     o = al(o + (size_t)bt->n_m * 6 * sizeof(double));
  const size_t o_b = o;     o = al(o + (size_t)bt->n_m * 3 * sizeof(double));
  const size_t o_Ci = o;    o = al(o + (size_t)bt->n_m * 6 * sizeof(double));
  const size_t o_Cib = o;   o = al(o + (size_t)bt->n_m * 3 * sizeof(double));
  const size_t o_W = o;     o = al(o + (size_t)bt->n_pair * 18 * sizeof(double));
  const size_t o_res = o;   o = al(o + (size_t)B * sizeof(ba_batch_result));
  bt->dev_bytes = o;
  if (hipSetDevice(h->device) != hipSuccess || hipMalloc((void **)&bt->dev, bt->dev_bytes) != hipSuccess) {
    delete bt;
    return fail("ba_batch_create: device allocation of " + std::to_string(o) + " bytes failed");
  }
  if (hipMemcpy(bt->dev, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(bt->dev);
    delete bt;
    return fail("ba_batch_create: upload failed");
  }
  ba::BatchDev &d = bt->d;
  char *D = bt->dev;
  d.prob = (const ba::BatchProb *)(D + o_prob);
  d.cams = (const double *)(D + o_cams);
  d.jopt = (const int32_t *)(D + o_jopt);
  d.opt_lm = (const int32_t *)(D + o_optlm);
  d.lobs = (const int4 *)(D + o_lobs);
  d.luv = (const double2 *)(D + o_luv);
  d.lm_ptr = (const int32_t *)(D + o_lmptr);
  d.pair_ptr = (const int32_t *)(D + o_pptr);
  d.pair_j = (const int32_t *)(D + o_pj);
  d.tab = (const int32_t *)(D + o_tab);
  d.pobs = (const int32_t *)(D + o_pobs);
  d.pobs_ptr = (const int32_t *)(D + o_poptr);
  d.poses = (double *)(D + o_poses);
  d.pts[0] = (double *)(D + o_pts);
  d.pts[1] = (double *)(D + o_pts1);
  d.C6 = (double *)(D + o_C);
  d.b3 = (double *)(D + o_b);
  d.Cinv6 = (double *)(D + o_Ci);
  d.Cinvb3 = (double *)(D + o_Cib);
  d.W18 = (double *)(D + o_W);
  d.res = (ba_batch_result *)(D + o_res);
  bt->lists0 = d;
  *out = bt;
  return 0;
}

void ba_batch_destroy(ba_batch *b) {
  if (!b) return;
  if (b->dev) (void)hipFree(b->dev);
  if (b->rows) (void)hipFree(b->rows);
  if (b->cov) (void)hipFree(b->cov);
  if (b->marg) (void)hipFree(b->marg);
  if (b->prior) (void)hipFree(b->prior);
  if (b->rel) (void)hipFree(b->rel);
  if (b->mask) (void)hipFree(b->mask);
  if (b->rep) (void)hipFree(b->rep);
  delete b;
}

int ba_batch_update_values(ba_batch *b, const double *T_jw12, const double *X3) {
  if (!b) return fail("ba_batch_update_values: null batch");
  HIP_TRY(hipSetDevice(b->h->device));
  hipStream_t s = b->h->stream;
  if (T_jw12)
    HIP_TRY(hipMemcpyAsync(b->d.poses, T_jw12, (size_t)b->n_pose * 12 * sizeof(double), hipMemcpyHostToDevice, s));
  if (X3)
    HIP_TRY(hipMemcpyAsync(b->d.pts[0], X3, (size_t)b->n_pt * 3 * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int ba_batch_get_poses(ba_batch *b, double *T_jw12) {
  if (!b || !T_jw12) return fail("ba_batch_get_poses: null argument");
  HIP_TRY(hipSetDevice(b->h->device));
  HIP_TRY(hipMemcpyAsync(T_jw12, b->d.poses, (size_t)b->n_pose * 12 * sizeof(double), hipMemcpyDeviceToHost,
                         b->h->stream));
  HIP_TRY(hipStreamSynchronize(b->h->stream));
  return 0;
}

int ba_batch_get_points(ba_batch *b, double *X3) {
  if (!b || !X3) return fail("ba_batch_get_points: null argument");
  HIP_TRY(hipSetDevice(b->h->device));
  HIP_TRY(hipMemcpyAsync(X3, b->d.pts[0], (size_t)b->n_pt * 3 * sizeof(double), hipMemcpyDeviceToHost,
                         b->h->stream));
  HIP_TRY(hipStreamSynchronize(b->h->stream));
  return 0;
}

int ba_batch_prior_check(int B, const int32_t *pose_off, const uint8_t *pose_fixed, const int32_t *prior_off,
                         const int32_t *prior_pose, const double *T_lin12, const double *H, const double *bvec,
                         const double *c) {
  if (B < 1) return fail("ba_batch_prior_check: B must be >= 1");
  if (!pose_off) return fail("ba_batch_prior_check: null pose_off");
  for (int p = 0; p < B; ++p)
    if (pose_off[p + 1] < pose_off[p]) return fail("ba_batch_prior_check: pose_off must not decrease");
  return prior_validate(
      "ba_batch_prior_check", B, [&](int p) { return pose_off[p + 1] - pose_off[p]; },
      [&](int p, int q) { return pose_fixed && pose_fixed[pose_off[p] + q] != 0; }, prior_off, prior_pose, T_lin12, H,
      bvec, c);
}

int ba_batch_set_prior(ba_batch *b, const int32_t *prior_off, const int32_t *prior_pose, const double *T_lin12,
                       const double *H, const double *bvec, const double *c) {
  if (!b) return fail("ba_batch_set_prior: null batch");
  const int B = b->B;
  if (prior_off &&
      prior_validate(
          "ba_batch_set_prior", B, [&](int p) { return (int)b->prob[p].n_pose; },
          [&](int p, int q) { return b->jopt[b->prob[p].pose0 + q] < 0; }, prior_off, prior_pose, T_lin12, H, bvec, c))
    return -1;
  HIP_TRY(hipSetDevice(b->h->device));
  if (b->prior) (void)hipFree(b->prior);
  b->prior = nullptr;
  b->prior_bytes = 0;
  b->prior_n = b->prior_K = 0;
  b->d.prior = nullptr;
  b->d.prior_j = nullptr;
  b->d.prior_T = b->d.prior_H = b->d.prior_b = nullptr;
  if (!prior_off) return 0;
  // the priors in effect (a problem over a limit keeps none), packed: one host image, one upload
  std::vector<ba::BatchPrior> rec(B);
  std::vector<int2> pj;
  std::vector<double> Tl, Hh, bb;
  int64_t ho = 0, n_on = 0, K_on = 0;
  for (int p = 0; p < B; ++p) {
    const int k0 = prior_off[p], K = prior_off[p + 1] - k0;
    const bool on = K > 0 && b->prob[p].status == 0;
    rec[p] = ba::BatchPrior{(int64_t)Hh.size(), (int64_t)pj.size(), on && c ? c[p] : 0.0, on ? K : 0, 0};
    if (on) {
      for (int t = 0; t < K; ++t) {
        const int q = prior_pose[k0 + t];
        pj.push_back(make_int2(q, b->jopt[b->prob[p].pose0 + q]));
      }
      Tl.insert(Tl.end(), T_lin12 + (int64_t)12 * k0, T_lin12 + (int64_t)12 * (k0 + K));
      Hh.insert(Hh.end(), H + ho, H + ho + (int64_t)36 * K * K);
      bb.insert(bb.end(), bvec + (int64_t)6 * k0, bvec + (int64_t)6 * (k0 + K));
      n_on += 1;
      K_on += K;
    }
    ho += (int64_t)36 * K * K;
  }
  if (n_on == 0) return 0;
  std::vector<char> blob;
  const size_t o_rec = put(blob, rec), o_pj = put(blob, pj), o_T = put(blob, Tl), o_H = put(blob, Hh),
               o_b = put(blob, bb);
  // the counts and the pointers are set last: after a failure below no prior is in effect
  if (hipMalloc((void **)&b->prior, blob.size()) != hipSuccess) {
    b->prior = nullptr;
    return fail("ba_batch_set_prior: device allocation of " + std::to_string(blob.size()) + " bytes failed");
  }
  if (hipMemcpy(b->prior, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(b->prior);
    b->prior = nullptr;
    return fail("ba_batch_set_prior: upload failed");
  }
  b->prior_bytes = blob.size();
  b->prior_n = n_on;
  b->prior_K = K_on;
  b->d.prior = (const ba::BatchPrior *)(b->prior + o_rec);
  b->d.prior_j = (const int2 *)(b->prior + o_pj);
  b->d.prior_T = (const double *)(b->prior + o_T);
  b->d.prior_H = (const double *)(b->prior + o_H);
  b->d.prior_b = (const double *)(b->prior + o_b);
  return 0;
}

int ba_batch_prior_info(ba_batch *b, int64_t out4[4]) {
  if (!b || !out4) return fail("ba_batch_prior_info: null argument");
  out4[0] = b->prior_n;
  out4[1] = b->prior_K;
  out4[2] = (int64_t)b->prior_bytes;
  out4[3] = 0;
  return 0;
}

int ba_batch_relative_check(int B, const int32_t *pose_off, const uint8_t *pose_fixed, const int32_t *rel_off,
                            const int32_t *rel_j, const int32_t *rel_k, const double *Z12, const double *Omega36) {
  if (B < 1) return fail("ba_batch_relative_check: B must be >= 1");
  if (!pose_off) return fail("ba_batch_relative_check: null pose_off");
  for (int p = 0; p < B; ++p)
    if (pose_off[p + 1] < pose_off[p]) return fail("ba_batch_relative_check: pose_off must not decrease");
  return relative_validate(
      "ba_batch_relative_check", B, [&](int p) { return pose_off[p + 1] - pose_off[p]; },
      [&](int p, int q) { return pose_fixed && pose_fixed[pose_off[p] + q] != 0; }, rel_off, rel_j, rel_k, Z12,
      Omega36);
}

int ba_batch_set_relative(ba_batch *b, const int32_t *rel_off, const int32_t *rel_j, const int32_t *rel_k,
                          const double *Z12, const double *Omega36) {
  if (!b) return fail("ba_batch_set_relative: null batch");
  const int B = b->B;
  if (rel_off &&
      relative_validate(
          "ba_batch_set_relative", B, [&](int p) { return (int)b->prob[p].n_pose; },
          [&](int p, int q) { return b->jopt[b->prob[p].pose0 + q] < 0; }, rel_off, rel_j, rel_k, Z12, Omega36))
    return -1;
  HIP_TRY(hipSetDevice(b->h->device));
  relative_drop(b);
  if (!rel_off) return 0;
  // the factors in effect (a problem over a limit keeps none), packed, with the two lists of
  // every problem in input order: one host image, one upload; the scratch follows it
  std::vector<ba::BatchRel> rec(B);
  std::vector<int4> jk;
  std::vector<double> Zs, Om;
  std::vector<int32_t> pptr, plist, bptr, blist;
  std::vector<int2> blk;
  ba::RelLists l;
  int64_t n_on = 0;
  for (int p = 0; p < B; ++p) {
    const ba::BatchProb &P = b->prob[p];
    const int f0 = rel_off[p], F = P.status == 0 ? rel_off[p + 1] - f0 : 0;
    rec[p] = ba::BatchRel{(int64_t)jk.size(), (int64_t)pptr.size(), (int64_t)plist.size(), (int64_t)blk.size(),
                          (int64_t)bptr.size(), (int64_t)blist.size(), F, 0};
    if (F == 0) continue;
    // the problem's lists, local to it; a coupled block's key is hi * N + lo, and H_jk is the
    // block (j, k): transposed where k is hi
    const int64_t N = P.N;
    ba::relative_build_lists(
        F, rel_j + f0, rel_k + f0, P.N, b->jopt.data() + P.pose0,
        [N](int32_t oj, int32_t ok) {
          return std::pair<int64_t, bool>(std::max(oj, ok) * N + std::min(oj, ok), oj < ok);
        },
        &l);
    for (int f = 0; f < F; ++f) jk.push_back(make_int4(l.jk[4 * f], l.jk[4 * f + 1], l.jk[4 * f + 2], l.jk[4 * f + 3]));
    Zs.insert(Zs.end(), Z12 + (int64_t)12 * f0, Z12 + (int64_t)12 * (f0 + F));
    Om.resize(Om.size() + (size_t)36 * F);
    for (int f = 0; f < F; ++f)
      ba::relative_mirror_omega(Omega36 + (int64_t)36 * (f0 + f), Om.data() + Om.size() - (size_t)36 * (F - f));
    rec[p].nblk = (int32_t)l.bkey.size();
    for (int64_t key : l.bkey) blk.push_back(make_int2((int)(key / N), (int)(key % N)));
    pptr.insert(pptr.end(), l.pptr.begin(), l.pptr.end());
    plist.insert(plist.end(), l.plist.begin(), l.plist.end());
    bptr.insert(bptr.end(), l.bptr.begin(), l.bptr.end());
    blist.insert(blist.end(), l.blist.begin(), l.blist.end());
    n_on += 1;
  }
  b->rel_off.assign(rel_off, rel_off + B + 1);
  b->rel_j.assign(rel_j, rel_j + rel_off[B]);
  b->rel_k.assign(rel_k, rel_k + rel_off[B]);
  if (n_on == 0) return 0;
  std::vector<char> blob;
  const size_t o_rec = put(blob, rec), o_jk = put(blob, jk), o_Z = put(blob, Zs), o_Om = put(blob, Om),
               o_pp = put(blob, pptr), o_pl = put(blob, plist), o_blk = put(blob, blk), o_bp = put(blob, bptr),
               o_bl = put(blob, blist), o_dev = put(blob, std::vector<ba::BatchRelDev>(1));
  const size_t o_scr = (blob.size() + 255) & ~(size_t)255;
  const size_t bytes = o_scr + jk.size() * ba::kRelScr * sizeof(double);
  // the counts and the pointers are set last: after a failure below no factor is in effect
  if (hipMalloc((void **)&b->rel, bytes) != hipSuccess) {
    b->rel = nullptr;
    relative_drop(b);
    return fail("ba_batch_set_relative: device allocation of " + std::to_string(bytes) + " bytes failed");
  }
  {
    ba::BatchRelDev rd;
    rd.rel = (const ba::BatchRel *)(b->rel + o_rec);
    rd.rel_jk = (const int4 *)(b->rel + o_jk);
    rd.rel_Z = (const double *)(b->rel + o_Z);
    rd.rel_Om = (const double *)(b->rel + o_Om);
    rd.rel_pptr = (const int32_t *)(b->rel + o_pp);
    rd.rel_plist = (const int32_t *)(b->rel + o_pl);
    rd.rel_blk = (const int2 *)(b->rel + o_blk);
    rd.rel_bptr = (const int32_t *)(b->rel + o_bp);
    rd.rel_blist = (const int32_t *)(b->rel + o_bl);
    rd.rel_scr = (double *)(b->rel + o_scr);
    std::memcpy(blob.data() + o_dev, &rd, sizeof(rd));
  }
  if (hipMemcpy(b->rel, blob.data(), blob.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(b->rel + o_scr, 0, bytes - o_scr) != hipSuccess) {
    relative_drop(b);
    return fail("ba_batch_set_relative: upload failed");
  }
  b->rel_bytes = bytes;
  b->rel_n = n_on;
  b->rel_F = (int64_t)jk.size();
  b->relp = (const ba::BatchRelDev *)(b->rel + o_dev);
  return 0;
}

int ba_batch_relative_info(ba_batch *b, int64_t out4[4]) {
  if (!b || !out4) return fail("ba_batch_relative_info: null argument");
  out4[0] = b->rel_n;
  out4[1] = b->rel_F;
  out4[2] = (int64_t)b->rel_bytes;
  out4[3] = 0;
  return 0;
}

int ba_batch_relative_marg_plan(ba_batch *b, const uint8_t *marg_pose, uint8_t *rel_leaves) {
  if (!b) return fail("ba_batch_relative_marg_plan: null batch");
  if (b->rel_off.empty() || b->rel_off[b->B] == 0) return 0;  // no factors: nothing to write
  if (!marg_pose || !rel_leaves) return fail("ba_batch_relative_marg_plan: null argument");
  for (int p = 0; p < b->B; ++p) {
    const ba::BatchProb &P = b->prob[p];
    for (int f = b->rel_off[p]; f < b->rel_off[p + 1]; ++f)
      rel_leaves[f] = P.status == 0 && (marg_pose[P.pose0 + b->rel_j[f]] || marg_pose[P.pose0 + b->rel_k[f]]) ? 1 : 0;
  }
  return 0;
}

int ba_batch_info(ba_batch *b, int64_t out8[8]) {
  if (!b || !out8) return fail("ba_batch_info: null argument");
  out8[0] = b->max_scratch;
  out8[1] = (int64_t)lds_bytes_of(b->npt_class);
  out8[2] = ba::kBatchMaxOpt;
  out8[3] = ba::kBatchMaxPoses;
  out8[4] = ba::kCamLds;
  out8[5] = 16 * b->npt_class;
  out8[6] = (int64_t)b->dev_bytes;
  out8[7] = b->B;
  return 0;
}

int ba_batch_scratch_bytes(ba_batch *b, int64_t *bytes) {
  if (!b || !bytes) return fail("ba_batch_scratch_bytes: null argument");
  for (int p = 0; p < b->B; ++p) bytes[p] = scratch_bytes_of(b->prob[p]);
  return 0;
}

int ba_batch_solve(ba_batch *b, const ba_options *opt, ba_iter_info *rows, int cap, ba_batch_result *res) {
  if (!b) return fail("ba_batch_solve: null batch");
  if (!opt) return fail("ba_batch_solve: null options");
  if (!res) return fail("ba_batch_solve: null result array");
  if (cap < 0) return fail("ba_batch_solve: cap must be >= 0");
  const int B = b->B;
  if (opt->max_num_iterations <= 0) {  // nothing changes, converged, no rows
    for (int p = 0; p < B; ++p) res[p] = ba_batch_result{0, b->prob[p].status ? 0 : 1, 0, b->prob[p].status, 0};
    return 0;
  }
  HIP_TRY(hipSetDevice(b->h->device));
  hipStream_t s = b->h->stream;
  const int dcap = rows ? cap : 0;
  const size_t n_rows = (size_t)B * (size_t)dcap;
  if (rows_reserve(b, n_rows)) return -1;
  ba::BatchDev d = b->d;
  d.rows = b->rows;
  d.cap = dcap;
  solve_launch(b, opt, d);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(res, d.res, (size_t)B * sizeof(ba_batch_result), hipMemcpyDeviceToHost, s));
  if (dcap > 0)
    HIP_TRY(hipMemcpyAsync(rows, b->rows, n_rows * sizeof(ba_iter_info), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int ba_batch_marg_plan_problem(int n_pose, const uint8_t *pose_fixed, const uint8_t *marg_pose, int n_pt,
                               const uint8_t *pt_fixed, int64_t n_obs, const int32_t *obs_pose, const int32_t *obs_pt,
                               int32_t *kept_pose, uint8_t *marg_pt) {
  if (n_pose < 0 || n_pt < 0 || n_obs < 0 || n_obs > INT32_MAX) return fail("ba_batch_marg_plan_problem: bad sizes");
  if (n_pose > 0 && !marg_pose) return fail("ba_batch_marg_plan_problem: null marg_pose");
  if (n_obs > 0 && (!obs_pose || !obs_pt)) return fail("ba_batch_marg_plan_problem: null observations");
  for (int64_t k = 0; k < n_obs; ++k)
    if (obs_pose[k] < 0 || obs_pose[k] >= n_pose || obs_pt[k] < 0 || obs_pt[k] >= n_pt)
      return fail("ba_batch_marg_plan_problem: observation " + std::to_string(k) + " out of range");
  int K = 0;
  for (int p = 0; p < n_pose; ++p)
    if (!(pose_fixed && pose_fixed[p]) && !marg_pose[p]) {
      if (kept_pose) kept_pose[K] = p;
      ++K;
    }
  if (marg_pt) {
    for (int q = 0; q < n_pt; ++q) marg_pt[q] = 0;
    for (int64_t k = 0; k < n_obs; ++k)
      if (marg_pose[obs_pose[k]] && !(pt_fixed && pt_fixed[obs_pt[k]])) marg_pt[obs_pt[k]] = 1;
  }
  return K;
}

int ba_batch_marg_layout(ba_batch *b, const uint8_t *marg_pose, int64_t *H_off, int64_t *b_off) {
  if (!b) return fail("ba_batch_marg_layout: null batch");
  if (!marg_pose && b->n_pose > 0) return fail("ba_batch_marg_layout: null marg_pose");
  if (!H_off || !b_off) return fail("ba_batch_marg_layout: null offsets");
  std::vector<ba::BatchMargProb> mp;
  marg_plan_batch(b, marg_pose, mp);
  for (int p = 0; p < b->B; ++p) {
    H_off[p] = mp[p].H_off;
    b_off[p] = mp[p].b_off;
  }
  H_off[b->B] = mp.back().H_off + (int64_t)36 * mp.back().K * mp.back().K;
  b_off[b->B] = mp.back().b_off + (int64_t)6 * mp.back().K;
  return 0;
}

int ba_batch_marginalize(ba_batch *b, double huber, const uint8_t *marg_pose, double *H, double *bvec,
                         uint8_t *marg_pt, ba_batch_marg_result *res) {
  if (!b) return fail("ba_batch_marginalize: null batch");
  if (!marg_pose && b->n_pose > 0) return fail("ba_batch_marginalize: null marg_pose");
  if (!res) return fail("ba_batch_marginalize: null result array");
  const int B = b->B;
  std::vector<ba::BatchMargProb> mp;
  const int tiles = marg_plan_batch(b, marg_pose, mp);
  const size_t nH = (size_t)(mp.back().H_off + (int64_t)36 * mp.back().K * mp.back().K);
  const size_t nb = (size_t)(mp.back().b_off + (int64_t)6 * mp.back().K);
  if (nH > 0 && !H) return fail("ba_batch_marginalize: null H");
  if (nb > 0 && !bvec) return fail("ba_batch_marginalize: null bvec");
  HIP_TRY(hipSetDevice(b->h->device));
  hipStream_t s = b->h->stream;
  // one buffer: H | b | marg_pt (zeroed) | marg_pose | plan (uploaded) | results
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_b = al(nH * sizeof(double)), o_sel = o_b + al(nb * sizeof(double));
  const size_t o_in = o_sel + al((size_t)b->n_pt), o_mp = al((size_t)b->n_pose);
  const size_t in_bytes = o_mp + al((size_t)B * sizeof(ba::BatchMargProb));
  const size_t o_res = o_in + in_bytes, bytes = o_res + al((size_t)B * sizeof(ba_batch_marg_result));
  if (bytes > b->marg_bytes) {
    if (b->marg) (void)hipFree(b->marg);
    b->marg = nullptr;
    b->marg_bytes = 0;
    HIP_TRY(hipMalloc((void **)&b->marg, bytes));
    b->marg_bytes = bytes;
  }
  std::vector<char> in(in_bytes, 0);
  if (b->n_pose > 0) std::memcpy(in.data(), marg_pose, (size_t)b->n_pose);
  std::memcpy(in.data() + o_mp, mp.data(), (size_t)B * sizeof(ba::BatchMargProb));
  ba::BatchMargOut o;
  o.H = (double *)b->marg;
  o.bvec = (double *)(b->marg + o_b);
  o.sel = (uint8_t *)(b->marg + o_sel);
  o.marg = (const uint8_t *)(b->marg + o_in);
  o.mp = (const ba::BatchMargProb *)(b->marg + o_in + o_mp);
  o.res = (ba_batch_marg_result *)(b->marg + o_res);
  o.huber = huber;
  HIP_TRY(hipMemsetAsync(b->marg, 0, o_in, s));  // unprocessed problems and unseen poses: exact zeros
  HIP_TRY(hipMemcpyAsync(b->marg + o_in, in.data(), in_bytes, hipMemcpyHostToDevice, s));
  if (b->relp)
    ba::batch_launch_rel(2, tiles <= 2 ? 2 : tiles <= 4 ? 4 : tiles <= 6 ? 6 : 7, B, s, &b->d, &o, b->relp);
  else if (tiles <= 2)
    hipLaunchKernelGGL(ba::k_ba_batch_marg<2>, dim3(B), dim3(ba::kBatchBlock), 0, s, b->d, o);
  else if (tiles <= 4)
    hipLaunchKernelGGL(ba::k_ba_batch_marg<4>, dim3(B), dim3(ba::kBatchBlock), 0, s, b->d, o);
  else if (tiles <= 6)
    hipLaunchKernelGGL(ba::k_ba_batch_marg<6>, dim3(B), dim3(ba::kBatchBlock), 0, s, b->d, o);
  else
    hipLaunchKernelGGL(ba::k_ba_batch_marg<7>, dim3(B), dim3(ba::kBatchBlock), 0, s, b->d, o);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(res, o.res, (size_t)B * sizeof(ba_batch_marg_result), hipMemcpyDeviceToHost, s));
  if (nH > 0) HIP_TRY(hipMemcpyAsync(H, o.H, nH * sizeof(double), hipMemcpyDeviceToHost, s));
  if (nb > 0) HIP_TRY(hipMemcpyAsync(bvec, o.bvec, nb * sizeof(double), hipMemcpyDeviceToHost, s));
  if (marg_pt && b->n_pt > 0) HIP_TRY(hipMemcpyAsync(marg_pt, o.sel, (size_t)b->n_pt, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int ba_batch_covariance(ba_batch *b, double huber, double *cov_pose36, double *cov_pt9, ba_batch_cov_result *res) {
  if (!b) return fail("ba_batch_covariance: null batch");
  if (!cov_pose36) return fail("ba_batch_covariance: null cov_pose36");
  if (!res) return fail("ba_batch_covariance: null result array");
  const int B = b->B;
  HIP_TRY(hipSetDevice(b->h->device));
  hipStream_t s = b->h->stream;
  if (!b->cov) {  // outputs of the call, kept with the object: pose blocks | point blocks | results
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    b->cov_pt_off = al((size_t)b->n_pose * 36 * sizeof(double));
    b->cov_res_off = b->cov_pt_off + al((size_t)b->n_pt * 9 * sizeof(double));
    b->cov_bytes = b->cov_res_off + al((size_t)B * sizeof(ba_batch_cov_result));
    HIP_TRY(hipMalloc((void **)&b->cov, b->cov_bytes));
  }
  ba::BatchCovOut o;
  o.pose36 = (double *)b->cov;
  o.pt9 = cov_pt9 ? (double *)(b->cov + b->cov_pt_off) : nullptr;
  o.res = (ba_batch_cov_result *)(b->cov + b->cov_res_off);
  o.huber = huber;
  HIP_TRY(hipMemsetAsync(b->cov, 0, b->cov_bytes, s));  // fixed members and unprocessed problems: exact zeros
  if (b->relp)
    ba::batch_launch_rel(1, b->npt_class, B, s, &b->d, &o, b->relp);
  else if (b->npt_class == 2)
    hipLaunchKernelGGL((ba::k_ba_batch_cov<2, false>), dim3(B), dim3(ba::kBatchBlock), 0, s, b->d, o);
  else if (b->npt_class == 4)
    hipLaunchKernelGGL((ba::k_ba_batch_cov<4, false>), dim3(B), dim3(ba::kBatchBlock), 0, s, b->d, o);
  else
    hipLaunchKernelGGL((ba::k_ba_batch_cov<6, false>), dim3(B), dim3(ba::kBatchBlock), 0, s, b->d, o);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(res, o.res, (size_t)B * sizeof(ba_batch_cov_result), hipMemcpyDeviceToHost, s));
  if (b->n_pose > 0)
    HIP_TRY(hipMemcpyAsync(cov_pose36, o.pose36, (size_t)b->n_pose * 36 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (cov_pt9 && b->n_pt > 0)
    HIP_TRY(hipMemcpyAsync(cov_pt9, o.pt9, (size_t)b->n_pt * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int ba_batch_cull_check(const ba_cull_options *c) {
  std::string err;
  if (ba::cull_validate_host(c ? &c->e2_max : nullptr, &err)) return fail("ba_batch_cull_check: " + err);
  return 0;
}

int ba_batch_obs_report(ba_batch *b, double huber, double *r2, double *e2, double *w, double *depth) {
  if (!b) return fail("ba_batch_obs_report: null batch");
  if (!r2 && !e2 && !w && !depth) return fail("ba_batch_obs_report: every output is null");
  if (b->n_obs == 0) return 0;
  HIP_TRY(hipSetDevice(b->h->device));
  hipStream_t s = b->h->stream;
  if (mask_ensure(b)) return -1;
  const size_t n = (size_t)b->n_obs;
  if (!b->rep) HIP_TRY(hipMalloc((void **)&b->rep, n * 5 * sizeof(double)));  // r2 | e2 | w | depth
  double *R = (double *)b->rep;
  hipLaunchKernelGGL(ba::k_ba_batch_obs_report, dim3((unsigned)((n + ba::kBatchBlock - 1) / ba::kBatchBlock)),
                     dim3(ba::kBatchBlock), 0, s, b->md, b->B, (int64_t)n, huber, r2 ? R : nullptr,
                     e2 ? R + 2 * n : nullptr, w ? R + 3 * n : nullptr, depth ? R + 4 * n : nullptr);
  HIP_TRY(hipGetLastError());
  if (r2) HIP_TRY(hipMemcpyAsync(r2, R, 2 * n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (e2) HIP_TRY(hipMemcpyAsync(e2, R + 2 * n, n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (w) HIP_TRY(hipMemcpyAsync(w, R + 3 * n, n * sizeof(double), hipMemcpyDeviceToHost, s));
  if (depth) HIP_TRY(hipMemcpyAsync(depth, R + 4 * n, n * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int ba_batch_set_obs_mask(ba_batch *b, const uint8_t *obs_on) {
  if (!b) return fail("ba_batch_set_obs_mask: null batch");
  HIP_TRY(hipSetDevice(b->h->device));
  hipStream_t s = b->h->stream;
  if (!obs_on) {  // the planned lists again; the flags read all on
    if (!b->mask) return 0;
    mask_point(b, false);
    HIP_TRY(hipMemsetAsync(b->md.on, 1, (size_t)b->n_obs, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
  }
  if (mask_ensure(b)) return -1;
  std::vector<uint8_t> on((size_t)b->n_obs);
  for (int64_t k = 0; k < b->n_obs; ++k) on[k] = obs_on[k] ? 1 : 0;
  if (b->n_obs > 0) HIP_TRY(hipMemcpyAsync(b->md.on, on.data(), on.size(), hipMemcpyHostToDevice, s));
  mask_apply_launch(b);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int ba_batch_get_obs_mask(ba_batch *b, uint8_t *obs_on) {
  if (!b || !obs_on) return fail("ba_batch_get_obs_mask: null argument");
  if (!b->mask) {
    std::memset(obs_on, 1, (size_t)b->n_obs);
    return 0;
  }
  if (b->n_obs == 0) return 0;
  HIP_TRY(hipSetDevice(b->h->device));
  HIP_TRY(hipMemcpyAsync(obs_on, b->md.on, (size_t)b->n_obs, hipMemcpyDeviceToHost, b->h->stream));
  HIP_TRY(hipStreamSynchronize(b->h->stream));
  return 0;
}

int ba_batch_cull(ba_batch *b, const ba_cull_options *c, ba_batch_cull_result *cres) {
  if (cull_refuse("ba_batch_cull", b, c, cres)) return -1;
  HIP_TRY(hipSetDevice(b->h->device));
  hipStream_t s = b->h->stream;
  if (mask_ensure(b)) return -1;
  cull_launch(b, c);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(cres, b->md.cres, (size_t)b->B * sizeof(ba_batch_cull_result), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

int ba_batch_solve_culled(ba_batch *b, const ba_options *first, const ba_options *second, const ba_cull_options *c,
                          ba_iter_info *rows, int cap, ba_batch_result *res_first, ba_batch_result *res,
                          ba_batch_cull_result *cres) {
  const char *who = "ba_batch_solve_culled";
  if (!b) return fail(std::string(who) + ": null batch");
  if (!first || !second) return fail(std::string(who) + ": null options");
  if (!res) return fail(std::string(who) + ": null result array");
  if (cull_refuse(who, b, c, cres)) return -1;
  std::string err;
  if (ba::solve_culled_validate_host(first->max_num_iterations, second->max_num_iterations, rows != nullptr, cap,
                                     &err))
    return fail(std::string(who) + ": " + err);
  const int B = b->B;
  HIP_TRY(hipSetDevice(b->h->device));
  hipStream_t s = b->h->stream;
  if (mask_ensure(b)) return -1;
  const int dcap = rows ? cap : 0, off = first->max_num_iterations;
  const size_t n_rows = (size_t)B * (size_t)dcap;
  if (rows_reserve(b, n_rows)) return -1;
  // stage 1 on the lists in effect, its results beside the mask; the cull; stage 2 on the
  // shadow lists, its rows after those of stage 1
  ba::BatchDev d = b->d;
  d.rows = b->rows;
  d.cap = dcap;
  d.res = b->res_first;
  solve_launch(b, first, d);
  HIP_TRY(hipGetLastError());
  cull_launch(b, c);
  HIP_TRY(hipGetLastError());
  d = b->d;
  d.rows = dcap ? b->rows + off : b->rows;
  d.cap = dcap;
  solve_launch(b, second, d);
  HIP_TRY(hipGetLastError());
  std::vector<ba_batch_result> r1((size_t)B);
  std::vector<ba_iter_info> hr(n_rows);
  HIP_TRY(hipMemcpyAsync(r1.data(), b->res_first, (size_t)B * sizeof(ba_batch_result), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(res, d.res, (size_t)B * sizeof(ba_batch_result), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(cres, b->md.cres, (size_t)B * sizeof(ba_batch_cull_result), hipMemcpyDeviceToHost, s));
  if (n_rows > 0) HIP_TRY(hipMemcpyAsync(hr.data(), b->rows, n_rows * sizeof(ba_iter_info), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int p = 0; p < B && dcap > 0; ++p) {  // the rows each stage wrote; those in between stay the caller's
    const size_t r0 = (size_t)p * dcap;
    const int n1 = std::min(r1[p].n_rows, off), n2 = std::min(res[p].n_rows, dcap - off);
    std::copy(hr.begin() + r0, hr.begin() + r0 + std::max(n1, 0), rows + r0);
    std::copy(hr.begin() + r0 + off, hr.begin() + r0 + off + std::max(n2, 0), rows + r0 + off);
  }
  if (res_first) std::copy(r1.begin(), r1.end(), res_first);
  return 0;
}

}  // extern "C"
