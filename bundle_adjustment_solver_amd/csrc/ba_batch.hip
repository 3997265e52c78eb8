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
// kernels (batch_prior_lin / batch_prior_offdiag / batch_prior_cost below).  H stays in
// global memory; the branch is uniform per workgroup and a problem without a prior executes
// none of it.
//
// Host side: ba_batch_create plans the structure once (stable landmark-major grouping,
// pair lists, last-writer marks, one upload); ba_batch_solve is one launch and one sync.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ba_chol_lds.h"
#include "ba_device_fn.h"
#include "ba_handle.h"

namespace ba {
namespace {

constexpr int kBatchBlock = 256;
constexpr int kBatchMaxOpt = 16;    // optimisable poses: 6 * 16 = kTailCols columns
constexpr int kBatchMaxPoses = 64;  // all poses: accepted + trial transforms in LDS (12 KiB)
constexpr int kBatchMaxBlk = kBatchMaxOpt * (kBatchMaxOpt + 1) / 2;
static_assert(6 * kBatchMaxOpt <= kTailCols, "the reduced system must fit the LDS image");

struct BatchProb {  // one problem: sizes and element offsets into the concatenated arrays
  int32_t n_cam, n_pose, N, n_pt, M, status, n_obs, P;
  int64_t cam0, pose0, pt0, obs0, pair0;  // cameras, poses, points, observations, pairs
  int64_t m0, tab0, pobs0, pptr0;         // opt landmarks, M*N table, pose-major list, its N+1 pointers
};

struct BatchPrior {  // the prior of one problem: K poses from pose k0 of the prior arrays
  int64_t H_off, k0;
  double c;
  int32_t K, pad_;
};

struct BatchDev {
  const BatchProb *prob;
  const double *cams;    // 16 per camera: fx fy cx cy R_cj t_cj
  double *poses;         // 12 per pose, in/out
  const int32_t *jopt;   // per pose: optimisable index or -1
  double *pts[2];        // 3 per point; [0] in/out, [1] the other parameter buffer
  const int32_t *opt_lm; // per optimisable landmark: its point (problem-local)
  const int4 *lobs;      // landmark-major: {camera, pose, point, pair << 1 | last writer, or -1}
  const double2 *luv;
  const int32_t *lm_ptr;   // per point (+1 per problem): first observation (problem-local)
  const int32_t *pair_ptr; // per optimisable landmark (+1 per problem): first pair
  const int32_t *pair_j;   // per pair: optimisable pose
  const int32_t *tab;      // per (optimisable landmark, optimisable pose): pair or -1
  const int32_t *pobs;     // per optimisable pose, landmark-major: observation (problem-local)
  const int32_t *pobs_ptr;
  // the pose priors (ba_batch_set_prior); prior == nullptr: none set
  const BatchPrior *prior;  // per problem
  const int2 *prior_j;      // per prior pose: {pose (problem-local), optimisable index}
  const double *prior_T;    // 12 per prior pose: T_lin
  const double *prior_H, *prior_b;
  // scratch
  double *C6, *b3, *Cinv6, *Cinvb3, *W18;
  DevIterRec *rows;
  int cap;
  ba_batch_result *res;
  // options (promoted as the handle path promotes them)
  double lambda0, huber, thr_step, thr_cost, dec_ratio, inc_ratio;
  int max_iter, gn;
};

template <int NPt>
struct BatchLds {
  static constexpr int nbt = 16 * NPt;
  static constexpr int LS = nbt + 16 + 1;
  double Lb[nbt * LS];
  double Eb[NPt][16 * kTailES];
  double xs[kTailCols];
  double cams[kCamLds * 16];
  double P[2][kBatchMaxPoses * 12];
  double A[kBatchMaxOpt * 36];
  double a[kBatchMaxOpt * 6];
  double pd[kTailCols], pg[kTailCols];  // prior: tangents delta, gradient g = b - H delta
  double red[8];
  double bc[4];  // trial cost, model estimate, sum |y|, sum |x| (thread 0 -> control step)
  DevCtrl ctrl;
  int32_t jopt[kBatchMaxPoses];
  uint8_t blk_j[kBatchMaxBlk], blk_k[kBatchMaxBlk];
};

// sum of residual norms over every observation of the problem at parameter buffer `sel`
template <class LDS>
__device__ __forceinline__ double batch_cost(const BatchDev &d, const BatchProb &pr, LDS &s, const int sel) {
  const int4 *ob = d.lobs + pr.obs0;
  const double2 *uv = d.luv + pr.obs0;
  const double *X = d.pts[sel] + pr.pt0 * 3;
  double acc = 0.0;
  for (int t = threadIdx.x; t < pr.n_obs; t += kBatchBlock) {
    const int4 r = ob[t];
    const double2 u = uv[t];
    const double *Xp = X + (size_t)r.z * 3;
    ObsGeom g;
    project(s.cams + r.x * 16, s.P[sel] + r.y * 12, Xp[0], Xp[1], Xp[2], u.x, u.y, g);
    acc += sqrt(g.r0 * g.r0 + g.r1 * g.r1);
  }
  return block_sum(acc, s.red);
}

// ---- the steps of one linearisation, shared by k_ba_batch and k_ba_batch_cov --------------
// landmark side (reference :811-828): one thread per optimisable landmark, its observations
// in insertion order; C_i, b_i and the cross block of a pair's LAST observation.
// sel (here and in the steps below): nullptr, or one byte per point of the problem; a
// landmark whose byte is 0 is left out of the linearisation (k_ba_batch_marg)
__device__ __forceinline__ void batch_landmark_pass(const int M, const int32_t *opt_lm, const int32_t *lm_ptr,
                                                    const int4 *ob, const double2 *uvp, const double *cams,
                                                    const double *Pc, const double *X, const double huber,
                                                    double *C6, double *b3, double *Wg,
                                                    const uint8_t *sel = nullptr) {
  const int tid = threadIdx.x;
  for (int i = tid; i < M; i += kBatchBlock) {
    const int q = opt_lm[i];
    if (sel && !sel[q]) continue;
    const double x0 = X[q * 3 + 0], x1 = X[q * 3 + 1], x2 = X[q * 3 + 2];
    double C[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
    const int o1 = lm_ptr[q + 1];
    for (int t = lm_ptr[q]; t < o1; ++t) {
      const int4 r = ob[t];
      const double2 u = uvp[t];
      const double *cam = cams + r.x * 16;
      const double *T = Pc + r.y * 12;
      ObsGeom g;
      project(cam, T, x0, x1, x2, u.x, u.y, g);
      double w, G[6], Rm[6];
      weight_and_G(cam, g, huber, w, G);
      make_R(G, T, Rm);
      const double wr0 = w * g.r0, wr1 = w * g.r1;
      C[0] += w * (Rm[0] * Rm[0] + Rm[3] * Rm[3]);
      C[1] += w * (Rm[0] * Rm[1] + Rm[3] * Rm[4]);
      C[2] += w * (Rm[0] * Rm[2] + Rm[3] * Rm[5]);
      C[3] += w * (Rm[1] * Rm[1] + Rm[4] * Rm[4]);
      C[4] += w * (Rm[1] * Rm[2] + Rm[4] * Rm[5]);
      C[5] += w * (Rm[2] * Rm[2] + Rm[5] * Rm[5]);
#pragma unroll
      for (int c = 0; c < 3; ++c) b[c] -= Rm[c] * wr0 + Rm[3 + c] * wr1;
      if (r.w >= 0 && (r.w & 1)) {  // the pair's last observation: B_ji = w Q^T R survives
        double Q[12];
        make_Q(G, g.Xij, Q);
        double *Wp = Wg + (size_t)(r.w >> 1) * 18;
#pragma unroll
        for (int rr = 0; rr < 6; ++rr)
#pragma unroll
          for (int c = 0; c < 3; ++c) Wp[rr * 3 + c] = w * (Q[rr] * Rm[c] + Q[6 + rr] * Rm[3 + c]);
      }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) C6[(size_t)i * 6 + k] = C[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) b3[(size_t)i * 3 + k] = b[k];
  }
}

// pose side (reference :789-809): one wave per optimisable pose, 27 wave sums -> A_j, a_j in LDS
__device__ __forceinline__ void batch_pose_pass(const int N, const int32_t *pp0, const int32_t *po, const int4 *ob,
                                                const double2 *uvp, const double *cams, const double *Pc,
                                                const double *X, const double huber, double *A, double *a,
                                                const uint8_t *sel = nullptr) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = wv; j < N; j += kBatchBlock / 64) {
    const int32_t *pp = pp0 + j;
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = 0.0;
    const int e1 = pp[1];
    for (int t = pp[0] + lane; t < e1; t += 64) {
      const int so = po[t];
      const int4 r = ob[so];
      if (sel && !sel[r.z]) continue;
      const double2 u = uvp[so];
      const double *cam = cams + r.x * 16;
      const double *Xp = X + (size_t)r.z * 3;
      ObsGeom g;
      project(cam, Pc + r.y * 12, Xp[0], Xp[1], Xp[2], u.x, u.y, g);
      double w, G[6], Q[12];
      weight_and_G(cam, g, huber, w, G);
      make_Q(G, g.Xij, Q);
      const double wr0 = w * g.r0, wr1 = w * g.r1;
      int k = 0;
#pragma unroll
      for (int rr = 0; rr < 6; ++rr)
#pragma unroll
        for (int c = rr; c < 6; ++c, ++k) acc[k] += (w * Q[rr]) * Q[c] + (w * Q[6 + rr]) * Q[6 + c];
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[21 + c] -= Q[c] * wr0 + Q[6 + c] * wr1;
    }
#pragma unroll
    for (int k = 0; k < 27; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
      int k = 0;
#pragma unroll
      for (int rr = 0; rr < 6; ++rr)
#pragma unroll
        for (int c = rr; c < 6; ++c, ++k) {
          A[j * 36 + rr * 6 + c] = acc[k];
          A[j * 36 + c * 6 + rr] = acc[k];
        }
#pragma unroll
      for (int c = 0; c < 6; ++c) a[j * 6 + c] = acc[21 + c];
    }
  }
}

// damp and invert (reference :846-856): C_i (1 + lambda) -> Cinv_i, Cinv_i b_i
__device__ __forceinline__ void batch_damp_invert(const int M, const double lp1, const double *C6, const double *b3,
                                                  double *Ci6, double *Cib3, const int32_t *opt_lm = nullptr,
                                                  const uint8_t *sel = nullptr) {
  const int tid = threadIdx.x;
  for (int i = tid; i < M; i += kBatchBlock) {
    if (sel && !sel[opt_lm[i]]) continue;
    double cd[6], ci[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) cd[k] = C6[(size_t)i * 6 + k];
    cd[0] *= lp1;
    cd[3] *= lp1;
    cd[5] *= lp1;
    spd3_inverse(cd, ci);
#pragma unroll
    for (int k = 0; k < 6; ++k) Ci6[(size_t)i * 6 + k] = ci[k];
    const double b0 = b3[(size_t)i * 3], b1 = b3[(size_t)i * 3 + 1], b2 = b3[(size_t)i * 3 + 2];
    Cib3[(size_t)i * 3 + 0] = ci[0] * b0 + ci[1] * b1 + ci[2] * b2;
    Cib3[(size_t)i * 3 + 1] = ci[1] * b0 + ci[3] * b1 + ci[4] * b2;
    Cib3[(size_t)i * 3 + 2] = ci[2] * b0 + ci[4] * b1 + ci[5] * b2;
  }
}

// reset the LDS image: zero, unit diagonal on the padding columns
template <int nbt, int LS>
__device__ __forceinline__ void batch_reset_image(double *Lb, const int n6) {
  const int tid = threadIdx.x;
  for (int e = tid; e < nbt * LS; e += kBatchBlock) {
    const int c = e / LS, r = e - c * LS;
    Lb[e] = (r == c && c >= n6) ? 1.0 : 0.0;  // unit diagonal on padding columns
  }
}

// Schur complement (reference :858-888): lower triangle of S and the reduced right-hand side
// into the LDS image; one thread per half 6x6 block, the landmarks in ascending order.
// PERM: col0 gives the first column of every optimisable pose in a permuted image (else pose
// j owns columns 6 j ..); a block whose poses j >= k land above the diagonal there is stored
// transposed, so that the lower triangle is complete either way
template <int nbt, int LS, bool PERM = false>
__device__ __forceinline__ void batch_schur(const int N, const int M, const double lp1, const int32_t *tab,
                                            const double *Ci6, const double *Cib3, const double *Wg,
                                            const uint8_t *blk_j, const uint8_t *blk_k, const double *A,
                                            const double *a, double *Lb, const int32_t *opt_lm = nullptr,
                                            const uint8_t *sel = nullptr, const uint8_t *col0 = nullptr) {
  const int tid = threadIdx.x, n6 = 6 * N;
  const int n_task = N * (N + 1);  // (block, half): rows 3h .. 3h+2 of block (j, k), j >= k
  for (int task = tid; task < n_task; task += kBatchBlock) {
    const int blk = task >> 1, h3 = (task & 1) * 3;
    const int j = blk_j[blk], k = blk_k[blk];
    double acc[18];
#pragma unroll
    for (int e = 0; e < 18; ++e) acc[e] = 0.0;
    for (int i = 0; i < M; ++i) {
      if (sel && !sel[opt_lm[i]]) continue;
      const int pj = tab[(size_t)i * N + j];
      const int pk = tab[(size_t)i * N + k];
      if (pj < 0 || pk < 0) continue;
      const double *I = Ci6 + (size_t)i * 6;
      const double i00 = I[0], i01 = I[1], i02 = I[2], i11 = I[3], i12 = I[4], i22 = I[5];
      const double *Wj = Wg + (size_t)pj * 18 + h3 * 3;
      double Wk[18];
#pragma unroll
      for (int e = 0; e < 18; ++e) Wk[e] = Wg[(size_t)pk * 18 + e];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double w0 = Wj[r * 3 + 0], w1 = Wj[r * 3 + 1], w2 = Wj[r * 3 + 2];
        // V_ji = B_ji Cinv_i (reference :862), never stored
        const double v0 = w0 * i00 + w1 * i01 + w2 * i02;
        const double v1 = w0 * i01 + w1 * i11 + w2 * i12;
        const double v2 = w0 * i02 + w1 * i12 + w2 * i22;
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[r * 6 + c] += v0 * Wk[c * 3 + 0] + v1 * Wk[c * 3 + 1] + v2 * Wk[c * 3 + 2];
      }
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        const int row = (PERM ? col0[j] : 6 * j) + h3 + r, col = (PERM ? col0[k] : 6 * k) + c;
        if (row < col && (!PERM || j == k)) continue;
        double av = 0.0;
        if (j == k) {
          av = A[j * 36 + (h3 + r) * 6 + c];
          if (h3 + r == c) av *= lp1;  // damped A_j (reference :833-844)
        }
        Lb[PERM && row < col ? row * LS + col : col * LS + row] = av - acc[r * 6 + c];
      }
  }
  for (int t = tid; t < n6; t += kBatchBlock) {  // rhs_j = a_j - sum_i B_ji (Cinv_i b_i)
    const int j = t / 6, r = t - 6 * j;
    double acc = 0.0;
    for (int i = 0; i < M; ++i) {
      if (sel && !sel[opt_lm[i]]) continue;
      const int pj = tab[(size_t)i * N + j];
      if (pj < 0) continue;
      const double *Wj = Wg + (size_t)pj * 18 + r * 3;
      const double *cb = Cib3 + (size_t)i * 3;
      acc += Wj[0] * cb[0] + Wj[1] * cb[1] + Wj[2] * cb[2];
    }
    Lb[(PERM ? col0[j] + r : t) * LS + nbt] = a[t] - acc;
  }
}

// ---- the pose prior of one problem, shared by the three kernels ---------------------------
// H(r, c) of the symmetric prior matrix, n = 6 K columns: only the lower triangle is read
__device__ __forceinline__ double prior_h(const double *H, const int n, const int r, const int c) {
  return r >= c ? H[(size_t)r * n + c] : H[(size_t)c * n + r];
}

// delta_t = se3_log(T_j T_lin,t^-1) of every prior pose at the poses P -> pd (no barrier)
__device__ __forceinline__ void batch_prior_delta(const int K, const int2 *pj, const double *Tl, const double *P,
                                                  double *pd) {
  for (int t = threadIdx.x; t < K; t += kBatchBlock) {
    const double *T = P + pj[t].x * 12, *L = Tl + (size_t)t * 12;
    double R[9], tt[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)  // R_j R_lin^T
        R[r * 3 + c] = T[r * 3 + 0] * L[c * 3 + 0] + T[r * 3 + 1] * L[c * 3 + 1] + T[r * 3 + 2] * L[c * 3 + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) tt[r] = T[9 + r] - (R[r * 3 + 0] * L[9] + R[r * 3 + 1] * L[10] + R[r * 3 + 2] * L[11]);
    se3_log(R, tt, pd + 6 * t);
  }
}

// Part 1, after batch_pose_pass: delta and g = b - H delta into LDS (one thread per row, the
// columns in ascending order), then H_jj into A_j and g_j into a_j: the prior's diagonal is
// damped with the rest of A_j.  Ends with a barrier.
__device__ __forceinline__ void batch_prior_lin(const int K, const int2 *pj, const double *Tl, const double *H,
                                                const double *b, const double *P, double *pd, double *pg, double *A,
                                                double *a) {
  const int tid = threadIdx.x, n = 6 * K;
  batch_prior_delta(K, pj, Tl, P, pd);
  __syncthreads();
  for (int r = tid; r < n; r += kBatchBlock) {
    double acc = 0.0;
    for (int c = 0; c < n; ++c) acc += prior_h(H, n, r, c) * pd[c];
    pg[r] = b[r] - acc;
  }
  __syncthreads();
  for (int e = tid; e < 36 * K; e += kBatchBlock) {
    const int t = e / 36, rc = e - 36 * t, r = rc / 6, c = rc - 6 * r;
    A[pj[t].y * 36 + rc] += prior_h(H, n, 6 * t + r, 6 * t + c);
  }
  for (int r = tid; r < n; r += kBatchBlock) {
    const int t = r / 6;
    a[pj[t].y * 6 + r - 6 * t] += pg[r];
  }
  __syncthreads();
}

// Part 2, after batch_schur and a barrier: the off-diagonal blocks H_tu, t > u, undamped,
// into the lower triangle of the image; one thread per element.  The prior poses ascend, so
// without a column map the block lies below the diagonal; with one (PERM) an element the
// map puts above it is stored transposed, as batch_schur<PERM> does.
template <int LS, bool PERM>
__device__ __forceinline__ void batch_prior_offdiag(const int K, const int2 *pj, const double *H, double *Lb,
                                                    const uint8_t *col0 = nullptr) {
  const int n = 6 * K, n_el = 18 * K * (K - 1);
  for (int e = threadIdx.x; e < n_el; e += kBatchBlock) {
    const int blk = e / 36, rc = e - 36 * blk, r = rc / 6, c = rc - 6 * r;
    int t = 1;
    while ((t * (t + 1)) / 2 <= blk) ++t;  // blk = t (t - 1) / 2 + u, u < t
    const int u = blk - (t * (t - 1)) / 2;
    const int jt = pj[t].y, ju = pj[u].y;
    const int row = (PERM ? col0[jt] : 6 * jt) + r, col = (PERM ? col0[ju] : 6 * ju) + c;
    Lb[PERM && row < col ? row * LS + col : col * LS + row] += H[(size_t)(6 * t + r) * n + 6 * u + c];
  }
}

// The prior's residual norm sqrt(max(0, d^T H d - 2 b^T d + c)) at the poses P; the rows are
// dealt to the threads, one block_sum; valid in thread 0.  pd is overwritten.
__device__ __forceinline__ double batch_prior_cost(const int K, const int2 *pj, const double *Tl, const double *H,
                                                   const double *b, const double c, const double *P, double *pd,
                                                   double *red) {
  const int n = 6 * K;
  __syncthreads();
  batch_prior_delta(K, pj, Tl, P, pd);
  __syncthreads();
  double e = 0.0;
  for (int r = threadIdx.x; r < n; r += kBatchBlock) {
    double acc = 0.0;
    for (int cc = 0; cc < n; ++cc) acc += prior_h(H, n, r, cc) * pd[cc];
    e += pd[r] * acc - 2.0 * (b[r] * pd[r]);
  }
  const double q = block_sum(e, red);
  return sqrt(fmax(0.0, q + c));
}

// the cross term 2 sum_{t > u} x_t^T H_tu x_u of the quadratic model, one row per thread
__device__ __forceinline__ double batch_prior_cross(const int K, const int2 *pj, const double *H, const double *xs) {
  const int n = 6 * K;
  double est = 0.0;
  for (int r = threadIdx.x; r < n; r += kBatchBlock) {
    const int t = r / 6;
    double acc = 0.0;
    for (int cc = 0; cc < 6 * t; ++cc) acc += H[(size_t)r * n + cc] * xs[6 * pj[cc / 6].y + cc % 6];
    est += 2.0 * (xs[6 * pj[t].y + r - 6 * t] * acc);
  }
  return est;
}

template <int NPt>
__global__ __launch_bounds__(kBatchBlock) void k_ba_batch(BatchDev d) {
  using LDS = BatchLds<NPt>;
  constexpr int nbt = LDS::nbt, LS = LDS::LS;
  __shared__ LDS s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const BatchProb pr = d.prob[blockIdx.x];
  ba_batch_result *res = d.res + blockIdx.x;
  if (pr.status != 0) {  // beyond a limit: not solved, nothing read or written but the result
    if (tid == 0) {
      res->n_iter = 0;
      res->converged = 0;
      res->n_rows = 0;
      res->status = pr.status;
      res->dropped_pivots = 0;
    }
    return;
  }
  const int N = pr.N, M = pr.M, n6 = 6 * N;
  // the prior of this problem (uniform per workgroup); Kp = 0: none
  const BatchPrior pp = d.prior ? d.prior[blockIdx.x] : BatchPrior{0, 0, 0.0, 0, 0};
  const int Kp = pp.K;
  const int2 *pj = d.prior_j + pp.k0;
  const double *pTl = d.prior_T + pp.k0 * 12, *pH = d.prior_H + pp.H_off, *pb = d.prior_b + pp.k0 * 6;
  double *Pg = d.poses + pr.pose0 * 12;
  double *X0 = d.pts[0] + pr.pt0 * 3, *X1 = d.pts[1] + pr.pt0 * 3;
  // ---- stage the problem; refuse non-finite parameters -------------------------------
  int bad_val = 0;
  for (int k = tid; k < pr.n_cam * 16; k += kBatchBlock) s.cams[k] = d.cams[pr.cam0 * 16 + k];
  for (int k = tid; k < pr.n_pose * 12; k += kBatchBlock) {
    const double v = Pg[k];
    s.P[0][k] = v;
    s.P[1][k] = v;  // fixed poses are never written again
    bad_val |= !isfinite(v);
  }
  for (int k = tid; k < pr.n_pose; k += kBatchBlock) s.jopt[k] = d.jopt[pr.pose0 + k];
  for (int k = tid; k < pr.n_pt * 3; k += kBatchBlock) {
    const double v = X0[k];
    X1[k] = v;  // fixed points are never written again
    bad_val |= !isfinite(v);
  }
  for (int k = tid; k < (int)(sizeof(s.Eb) / sizeof(double)); k += kBatchBlock) (&s.Eb[0][0])[k] = 0.0;
  if (tid == 0) {
    int b = 0;
    for (int j = 0; j < N; ++j)
      for (int k = 0; k <= j; ++k, ++b) {
        s.blk_j[b] = (uint8_t)j;
        s.blk_k[b] = (uint8_t)k;
      }
    res->dropped_pivots = 0;
    DevCtrl &c = s.ctrl;
    c.lambda = d.lambda0;
    c.huber = d.huber;
    c.thr_step = d.thr_step;
    c.thr_cost = d.thr_cost;
    c.dec_ratio = d.dec_ratio;
    c.inc_ratio = d.inc_ratio;
    c.max_iter = d.max_iter;
    c.gn = d.gn;
    c.cur = 0;
    c.lcur = 0;
    c.tcur = c.tlcur = 0;
    c.done = 0;
    c.iter = 0;
    c.converged = 0;
  }
  if (__syncthreads_or(bad_val)) {
    if (tid == 0) {
      res->n_iter = 0;
      res->converged = 0;
      res->n_rows = 0;
      res->status = 1;
    }
    return;
  }
  // ---- initial cost (reference :707-708) ----------------------------------------------
  {
    double c0 = batch_cost(d, pr, s, 0);
    if (Kp) {
      const double pc = batch_prior_cost(Kp, pj, pTl, pH, pb, pp.c, s.P[0], s.pd, s.red);
      c0 += pc;
    }
    if (tid == 0) {
      s.ctrl.prev_cost = c0;
      s.ctrl.t_last = wall_clock64();
    }
  }
  __syncthreads();
  const int4 *ob = d.lobs + pr.obs0;
  const double2 *uvp = d.luv + pr.obs0;
  const int32_t *lm_ptr = d.lm_ptr + pr.pt0 + blockIdx.x;
  const int32_t *opt_lm = d.opt_lm + pr.m0;
  const int32_t *pair_ptr = d.pair_ptr + pr.m0 + blockIdx.x;
  const int32_t *pair_j = d.pair_j + pr.pair0;
  const int32_t *tab = d.tab + pr.tab0;
  double *C6 = d.C6 + pr.m0 * 6, *b3 = d.b3 + pr.m0 * 3;
  double *Ci6 = d.Cinv6 + pr.m0 * 6, *Cib3 = d.Cinvb3 + pr.m0 * 3;
  double *Wg = d.W18 + pr.pair0 * 18;
  int cur = 0;
  bool need_lin = true;
  const double huber = d.huber;
  while (true) {
    const double *X = cur ? X1 : X0;
    double *Xt = cur ? X0 : X1;
    const double *Pc = s.P[cur];
    double *Pt = s.P[cur ^ 1];
    const double lp1 = 1.0 + s.ctrl.lambda;
    if (need_lin) {
      batch_landmark_pass(M, opt_lm, lm_ptr, ob, uvp, s.cams, Pc, X, huber, C6, b3, Wg);
      batch_pose_pass(N, d.pobs_ptr + pr.pptr0, d.pobs + pr.pobs0, ob, uvp, s.cams, Pc, X, huber, s.A, s.a);
      __syncthreads();
      if (Kp) batch_prior_lin(Kp, pj, pTl, pH, pb, Pc, s.pd, s.pg, s.A, s.a);
    }
    // ---- damp and invert (reference :846-856); reset the LDS image --------------------
    batch_damp_invert(M, lp1, C6, b3, Ci6, Cib3);
    batch_reset_image<nbt, LS>(s.Lb, n6);
    __syncthreads();
    // ---- Schur complement (reference :858-888), lower triangle, into the LDS image ----
    batch_schur<nbt, LS>(N, M, lp1, tab, Ci6, Cib3, Wg, s.blk_j, s.blk_k, s.A, s.a, s.Lb);
    __syncthreads();
    if (Kp > 1) {
      batch_prior_offdiag<LS, false>(Kp, pj, pH, s.Lb);
      __syncthreads();
    }
    // ---- reduced solve (reference :905) ------------------------------------------------
    chol_lds_factor_solve<NPt, false, LS>(s.Lb, s.Eb, s.xs, &res->dropped_pivots);
    __syncthreads();
    // ---- back-substitution, trial point, model, step norms (reference :910-963) -------
    double est = 0.0, sy = 0.0, estp = 0.0, sx = 0.0;
    for (int i = tid; i < M; i += kBatchBlock) {
      double u[3] = {0, 0, 0};
      const int p1 = pair_ptr[i + 1];
      for (int p = pair_ptr[i]; p < p1; ++p) {
        const double *xj = s.xs + 6 * pair_j[p];
        const double *W = Wg + (size_t)p * 18;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double v = 0.0;
#pragma unroll
          for (int r = 0; r < 6; ++r) v += W[r * 3 + c] * xj[r];
          u[c] += v;
        }
      }
      const double *I = Ci6 + (size_t)i * 6;
      const double *cb = Cib3 + (size_t)i * 3;
      const double y0 = cb[0] - (I[0] * u[0] + I[1] * u[1] + I[2] * u[2]);
      const double y1 = cb[1] - (I[1] * u[0] + I[3] * u[1] + I[4] * u[2]);
      const double y2 = cb[2] - (I[2] * u[0] + I[4] * u[1] + I[5] * u[2]);
      const int q = opt_lm[i];
      Xt[q * 3 + 0] = X[q * 3 + 0] + y0;
      Xt[q * 3 + 1] = X[q * 3 + 1] + y1;
      Xt[q * 3 + 2] = X[q * 3 + 2] + y2;
      const double *C = C6 + (size_t)i * 6;
      const double *b = b3 + (size_t)i * 3;
      const double c00 = C[0] * lp1, c11 = C[3] * lp1, c22 = C[5] * lp1;  // damped C_i (reference :447)
      const double r0 = y0 * c00 + y1 * C[1] + y2 * C[2];
      const double r1 = y0 * C[1] + y1 * c11 + y2 * C[4];
      const double r2 = y0 * C[2] + y1 * C[4] + y2 * c22;
      est += (b[0] * y0 + b[1] * y1 + b[2] * y2) + (r0 * y0 + r1 * y1 + r2 * y2) +
             2.0 * (y0 * u[0] + y1 * u[1] + y2 * u[2]);
      sy += sqrt(y0 * y0 + y1 * y1 + y2 * y2);
    }
    for (int p = tid; p < pr.n_pose; p += kBatchBlock) {
      const int j = s.jopt[p];
      if (j < 0) continue;
      const double *xj = s.xs + 6 * j;
      const double v0 = xj[0], v1 = xj[1], v2 = xj[2], w0 = xj[3], w1 = xj[4], w2 = xj[5];
      double dR[9], dt[3];
      se3_exp(v0, v1, v2, w0, w1, w2, dR, dt);
      const double *T = Pc + p * 12;
      double *To = Pt + p * 12;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
          To[r * 3 + c] = dR[r * 3 + 0] * T[0 * 3 + c] + dR[r * 3 + 1] * T[1 * 3 + c] + dR[r * 3 + 2] * T[2 * 3 + c];
        To[9 + r] = dR[r * 3 + 0] * T[9] + dR[r * 3 + 1] * T[10] + dR[r * 3 + 2] * T[11] + dt[r];
      }
      const double *aj = s.a + j * 6, *Aj = s.A + j * 36;
      double e = 0.0;
#pragma unroll
      for (int r = 0; r < 6; ++r) e += aj[r] * xj[r];
      double qd = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double rowc = 0.0;
#pragma unroll
        for (int r = 0; r < 6; ++r) rowc += xj[r] * (r == c ? Aj[r * 6 + c] * lp1 : Aj[r * 6 + c]);
        qd += rowc * xj[c];
      }
      estp += e + qd;
      sx += sqrt(v0 * v0 + v1 * v1 + v2 * v2 + w0 * w0 + w1 * w1 + w2 * w2);
    }
    if (Kp > 1) estp += batch_prior_cross(Kp, pj, pH, s.xs);
    block_sum2(est, sy, s.red);
    if (tid == 0) {
      s.bc[1] = est;
      s.bc[2] = sy;
    }
    block_sum2(estp, sx, s.red);
    if (tid == 0) {
      s.bc[1] += estp;
      s.bc[3] = sx;
    }
    __syncthreads();  // the trial parameters are complete
    // ---- trial cost, trust region, convergence, log row (reference :928-1007) ---------
    double tc = batch_cost(d, pr, s, cur ^ 1);
    if (Kp) {
      const double pc = batch_prior_cost(Kp, pj, pTl, pH, pb, pp.c, Pt, s.pd, s.red);
      tc += pc;
    }
    if (tid == 0)
      lm_control_step(&s.ctrl, d.rows + (size_t)blockIdx.x * d.cap, d.cap, (double)pr.n_obs, N + M, tc, s.bc[1],
                      s.bc[2], s.bc[3]);
    __syncthreads();
    const int ncur = s.ctrl.cur;
    need_lin = ncur != cur;  // rejected: the undamped blocks still belong to the accepted point
    cur = ncur;
    if (s.ctrl.done) break;
    __syncthreads();
  }
  __syncthreads();
  // ---- write back: poses, and the points if the accepted buffer is the second one ------
  for (int k = tid; k < pr.n_pose * 12; k += kBatchBlock) Pg[k] = s.P[cur][k];
  if (cur)
    for (int k = tid; k < pr.n_pt * 3; k += kBatchBlock) X0[k] = X1[k];
  if (tid == 0) {
    res->n_iter = s.ctrl.iter;
    res->converged = s.ctrl.converged;
    res->n_rows = s.ctrl.iter;
    res->status = 0;
  }
}

// ---- covariance blocks of every problem (ba_batch_covariance) -----------------------------
// The LDS of the covariance kernel: the image, the tile inverses and one pose set; neither
// the trial poses nor the controller of BatchLds.
template <int NPt>
struct BatchCovLds {
  static constexpr int nbt = 16 * NPt;
  static constexpr int LS = nbt + 16 + 1;
  double Lb[nbt * LS];
  double Eb[NPt][16 * kTailES];
  double xs[kTailCols];
  double cams[kCamLds * 16];
  double P[kBatchMaxPoses * 12];
  double A[kBatchMaxOpt * 36];
  double a[kBatchMaxOpt * 6];
  double pd[kTailCols], pg[kTailCols];  // prior: tangents delta, gradient g = b - H delta
  int32_t jopt[kBatchMaxPoses];
  uint8_t blk_j[kBatchMaxBlk], blk_k[kBatchMaxBlk];
};

struct BatchCovOut {
  double *pose36;  // 36 per pose of the batch (zeroed before the launch)
  double *pt9;     // 9 per point of the batch, or nullptr
  ba_batch_cov_result *res;
  double huber;
};

// One workgroup per problem: linearise at the held values with lambda = 0, Schur complement
// and Cholesky factor in LDS as k_ba_batch does, S^-1 in place (chol_lds_inverse), then
//   pose block      [S^-1]_jj                                   one thread per element
//   landmark block  Cinv_i + sum_jk Y_j^T [S^-1]_jk Y_k,        one thread per landmark,
//                   Y_j = W_ji Cinv_i                           its pairs in ascending pose order
// Every block is read from the lower triangle of S^-1 and mirrored: symmetric to the bit.
// The outputs were zeroed by the host: fixed members, and every block of a problem that is
// not processed (status 1 or 2), stay exactly zero.  Y_j overwrites W_ji in the scratch.
template <int NPt>
__global__ __launch_bounds__(kBatchBlock) void k_ba_batch_cov(BatchDev d, BatchCovOut o) {
  using LDS = BatchCovLds<NPt>;
  constexpr int nbt = LDS::nbt, LS = LDS::LS;
  __shared__ LDS s;
  const int tid = threadIdx.x;
  const BatchProb pr = d.prob[blockIdx.x];
  ba_batch_cov_result *res = o.res + blockIdx.x;
  if (pr.status != 0) {
    if (tid == 0) {
      res->status = pr.status;
      res->dropped_pivots = 0;
    }
    return;
  }
  const int N = pr.N, M = pr.M, n6 = 6 * N;
  // the prior of this problem (uniform per workgroup); Kp = 0: none
  const BatchPrior pp = d.prior ? d.prior[blockIdx.x] : BatchPrior{0, 0, 0.0, 0, 0};
  const int Kp = pp.K;
  const int2 *pj = d.prior_j + pp.k0;
  const double *pTl = d.prior_T + pp.k0 * 12, *pH = d.prior_H + pp.H_off, *pb = d.prior_b + pp.k0 * 6;
  const double *Pg = d.poses + pr.pose0 * 12;
  const double *X = d.pts[0] + pr.pt0 * 3;
  // ---- stage the problem; refuse non-finite parameters -------------------------------
  int bad_val = 0;
  for (int k = tid; k < pr.n_cam * 16; k += kBatchBlock) s.cams[k] = d.cams[pr.cam0 * 16 + k];
  for (int k = tid; k < pr.n_pose * 12; k += kBatchBlock) {
    const double v = Pg[k];
    s.P[k] = v;
    bad_val |= !isfinite(v);
  }
  for (int k = tid; k < pr.n_pose; k += kBatchBlock) s.jopt[k] = d.jopt[pr.pose0 + k];
  for (int k = tid; k < pr.n_pt * 3; k += kBatchBlock) bad_val |= !isfinite(X[k]);
  for (int k = tid; k < (int)(sizeof(s.Eb) / sizeof(double)); k += kBatchBlock) (&s.Eb[0][0])[k] = 0.0;
  if (tid == 0) {
    int b = 0;
    for (int j = 0; j < N; ++j)
      for (int k = 0; k <= j; ++k, ++b) {
        s.blk_j[b] = (uint8_t)j;
        s.blk_k[b] = (uint8_t)k;
      }
    res->dropped_pivots = 0;
  }
  if (__syncthreads_or(bad_val)) {
    if (tid == 0) res->status = 1;
    return;
  }
  const int4 *ob = d.lobs + pr.obs0;
  const double2 *uvp = d.luv + pr.obs0;
  const int32_t *lm_ptr = d.lm_ptr + pr.pt0 + blockIdx.x;
  const int32_t *opt_lm = d.opt_lm + pr.m0;
  const int32_t *pair_ptr = d.pair_ptr + pr.m0 + blockIdx.x;
  const int32_t *pair_j = d.pair_j + pr.pair0;
  double *C6 = d.C6 + pr.m0 * 6, *b3 = d.b3 + pr.m0 * 3;
  double *Ci6 = d.Cinv6 + pr.m0 * 6, *Cib3 = d.Cinvb3 + pr.m0 * 3;
  double *Wg = d.W18 + pr.pair0 * 18;
  // ---- linearise, lambda = 0; Schur complement; factor; invert --------------------------
  batch_landmark_pass(M, opt_lm, lm_ptr, ob, uvp, s.cams, s.P, X, o.huber, C6, b3, Wg);
  batch_pose_pass(N, d.pobs_ptr + pr.pptr0, d.pobs + pr.pobs0, ob, uvp, s.cams, s.P, X, o.huber, s.A, s.a);
  __syncthreads();
  if (Kp) batch_prior_lin(Kp, pj, pTl, pH, pb, s.P, s.pd, s.pg, s.A, s.a);
  batch_damp_invert(M, 1.0, C6, b3, Ci6, Cib3);
  batch_reset_image<nbt, LS>(s.Lb, n6);
  __syncthreads();
  batch_schur<nbt, LS>(N, M, 1.0, d.tab + pr.tab0, Ci6, Cib3, Wg, s.blk_j, s.blk_k, s.A, s.a, s.Lb);
  __syncthreads();
  if (Kp > 1) {
    batch_prior_offdiag<LS, false>(Kp, pj, pH, s.Lb);
    __syncthreads();
  }
  chol_lds_factor_solve<NPt, false, LS>(s.Lb, s.Eb, s.xs, &res->dropped_pivots);
  __syncthreads();
  chol_lds_inverse<NPt, LS>(s.Lb, s.Eb);  // ends with a barrier: the lower triangle holds S^-1
  // ---- pose blocks: the diagonal of S^-1 ------------------------------------------------
  for (int e = tid; e < pr.n_pose * 36; e += kBatchBlock) {
    const int p = e / 36, rc = e - 36 * p, r = rc / 6, c = rc - 6 * r;
    const int j = s.jopt[p];
    if (j < 0) continue;
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    o.pose36[(size_t)(pr.pose0 + p) * 36 + rc] = s.Lb[(6 * j + lo) * LS + 6 * j + hi];
  }
  if (!o.pt9) {
    if (tid == 0) res->status = 0;
    return;
  }
  // ---- landmark blocks ------------------------------------------------------------------
  for (int i = tid; i < M; i += kBatchBlock) {
    const double *I = Ci6 + (size_t)i * 6;
    const double i00 = I[0], i01 = I[1], i02 = I[2], i11 = I[3], i12 = I[4], i22 = I[5];
    const int p0 = pair_ptr[i], p1 = pair_ptr[i + 1];
    for (int p = p0; p < p1; ++p) {  // Y_j = W_ji Cinv_i in place
      double *W = Wg + (size_t)p * 18;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        const double w0 = W[r * 3 + 0], w1 = W[r * 3 + 1], w2 = W[r * 3 + 2];
        W[r * 3 + 0] = w0 * i00 + w1 * i01 + w2 * i02;
        W[r * 3 + 1] = w0 * i01 + w1 * i11 + w2 * i12;
        W[r * 3 + 2] = w0 * i02 + w1 * i12 + w2 * i22;
      }
    }
    double acc[6] = {0, 0, 0, 0, 0, 0};  // (00 01 02 11 12 22)
    for (int pa = p0; pa < p1; ++pa) {
      const int j6 = 6 * pair_j[pa];
      double T[18];  // sum_k [S^-1]_jk Y_k
#pragma unroll
      for (int e = 0; e < 18; ++e) T[e] = 0.0;
      for (int pb = p0; pb < p1; ++pb) {
        const int k6 = 6 * pair_j[pb];
        double Y[18];
#pragma unroll
        for (int e = 0; e < 18; ++e) Y[e] = Wg[(size_t)pb * 18 + e];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
          for (int c = 0; c < 6; ++c) {
            const int row = j6 + r, col = k6 + c;
            const double sv = row >= col ? s.Lb[col * LS + row] : s.Lb[row * LS + col];
#pragma unroll
            for (int q = 0; q < 3; ++q) T[r * 3 + q] += sv * Y[c * 3 + q];
          }
      }
      double Y[18];
#pragma unroll
      for (int e = 0; e < 18; ++e) Y[e] = Wg[(size_t)pa * 18 + e];
      int k = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b, ++k) {
          double v = 0.0;
#pragma unroll
          for (int r = 0; r < 6; ++r) v += Y[r * 3 + a] * T[r * 3 + b];
          acc[k] += v;
        }
    }
    double *out = o.pt9 + (size_t)(pr.pt0 + opt_lm[i]) * 9;
    const double c00 = i00 + acc[0], c01 = i01 + acc[1], c02 = i02 + acc[2];
    const double c11 = i11 + acc[3], c12 = i12 + acc[4], c22 = i22 + acc[5];
    out[0] = c00; out[1] = c01; out[2] = c02;
    out[3] = c01; out[4] = c11; out[5] = c12;
    out[6] = c02; out[7] = c12; out[8] = c22;
  }
  if (tid == 0) res->status = 0;
}

// ---- marginalisation prior of every problem (ba_batch_marginalize) ------------------------
// The LDS of the marginalisation kernel: BatchCovLds without the solution vector, plus the
// marking and the column map.  NPt = 7 (112 columns) holds the widest image a problem within
// the limits can ask for: 16 ceil(6 m / 16) + 6 (N - m) <= 110 for N <= 16.
template <int NPt>
struct BatchMargLds {
  static constexpr int nbt = 16 * NPt;
  static constexpr int LS = nbt + 16 + 1;
  double Lb[nbt * LS];
  double Eb[NPt][16 * kTailES];
  double cams[kCamLds * 16];
  double P[kBatchMaxPoses * 12];
  double A[kBatchMaxOpt * 36];
  double a[kBatchMaxOpt * 6];
  double pd[kTailCols], pg[kTailCols];  // prior: tangents delta, gradient g = b - H delta
  int32_t jopt[kBatchMaxPoses];
  int32_t n_sel;
  uint8_t marg[kBatchMaxPoses];
  uint8_t col0[kBatchMaxOpt];
  uint8_t blk_j[kBatchMaxBlk], blk_k[kBatchMaxBlk];
};

struct BatchMargProb {  // the host's plan of one problem for this marking
  int64_t H_off, b_off;  // element offsets of its outputs
  int32_t K, m;          // kept poses; marked optimisable poses
};

struct BatchMargOut {
  const BatchMargProb *mp;
  const uint8_t *marg;  // per pose of the batch: marked
  double *H, *bvec;     // zeroed before the launch
  uint8_t *sel;         // per point of the batch: in L (zeroed before the launch)
  ba_batch_marg_result *res;
  double huber;
};

// One workgroup per problem.  L = the optimisable landmarks a marked pose observes, decided
// by the thread that owns the landmark; the linearisation of k_ba_batch_cov restricted to L
// (lambda = 0); the Schur complement into a permuted image: the m marked optimisable poses
// first, padded with unit-diagonal columns to T = ceil(6 m / 16) tiles, the K kept poses from
// column 16 T on in ascending order.  chol_lds_partial eliminates the T tiles; what it leaves
// from column 16 T on is the prior: H is read from the lower triangle and mirrored, b from
// the rhs row.  The outputs were zeroed by the host: a problem that is not processed
// (status 1 or 2) leaves them zero.
template <int NPt>
__global__ __launch_bounds__(kBatchBlock) void k_ba_batch_marg(BatchDev d, BatchMargOut o) {
  using LDS = BatchMargLds<NPt>;
  constexpr int nbt = LDS::nbt, LS = LDS::LS;
  __shared__ LDS s;
  const int tid = threadIdx.x;
  const BatchProb pr = d.prob[blockIdx.x];
  const BatchMargProb mp = o.mp[blockIdx.x];
  ba_batch_marg_result *res = o.res + blockIdx.x;
  if (tid == 0) {
    res->dropped_pivots = 0;
    res->n_kept = mp.K;
    res->n_marg_pose = mp.m;
    res->n_marg_pt = 0;
  }
  if (pr.status != 0) {
    if (tid == 0) res->status = pr.status;
    return;
  }
  const int N = pr.N, M = pr.M, K = mp.K, K6 = 6 * K;
  // the prior of this problem (uniform per workgroup); Kp = 0: none
  const BatchPrior pp = d.prior ? d.prior[blockIdx.x] : BatchPrior{0, 0, 0.0, 0, 0};
  const int Kp = pp.K;
  const int2 *pj = d.prior_j + pp.k0;
  const double *pTl = d.prior_T + pp.k0 * 12, *pH = d.prior_H + pp.H_off, *pb = d.prior_b + pp.k0 * 6;
  const int T = (6 * mp.m + 15) >> 4;
  const double *Pg = d.poses + pr.pose0 * 12;
  const double *X = d.pts[0] + pr.pt0 * 3;
  // ---- stage the problem; refuse non-finite parameters -------------------------------
  int bad_val = 0;
  for (int k = tid; k < pr.n_cam * 16; k += kBatchBlock) s.cams[k] = d.cams[pr.cam0 * 16 + k];
  for (int k = tid; k < pr.n_pose * 12; k += kBatchBlock) {
    const double v = Pg[k];
    s.P[k] = v;
    bad_val |= !isfinite(v);
  }
  for (int k = tid; k < pr.n_pose; k += kBatchBlock) {
    s.jopt[k] = d.jopt[pr.pose0 + k];
    s.marg[k] = o.marg[pr.pose0 + k];
  }
  for (int k = tid; k < pr.n_pt * 3; k += kBatchBlock) bad_val |= !isfinite(X[k]);
  for (int k = tid; k < (int)(sizeof(s.Eb) / sizeof(double)); k += kBatchBlock) (&s.Eb[0][0])[k] = 0.0;
  if (tid == 0) s.n_sel = 0;
  if (__syncthreads_or(bad_val)) {
    if (tid == 0) res->status = 1;
    return;
  }
  if (tid == 0) {
    int b = 0;
    for (int j = 0; j < N; ++j)
      for (int k = 0; k <= j; ++k, ++b) {
        s.blk_j[b] = (uint8_t)j;
        s.blk_k[b] = (uint8_t)k;
      }
    int cm = 0, ck = 16 * T;  // the column map: marked poses from 0, kept poses from 16 T
    for (int p = 0; p < pr.n_pose; ++p) {
      const int j = s.jopt[p];
      if (j < 0) continue;
      if (s.marg[p]) {
        s.col0[j] = (uint8_t)cm;
        cm += 6;
      } else {
        s.col0[j] = (uint8_t)ck;
        ck += 6;
      }
    }
  }
  const int4 *ob = d.lobs + pr.obs0;
  const double2 *uvp = d.luv + pr.obs0;
  const int32_t *lm_ptr = d.lm_ptr + pr.pt0 + blockIdx.x;
  const int32_t *opt_lm = d.opt_lm + pr.m0;
  uint8_t *sel = o.sel + pr.pt0;
  // ---- L: an optimisable landmark with an observation from a marked pose -----------------
  int n_sel = 0;
  for (int i = tid; i < M; i += kBatchBlock) {
    const int q = opt_lm[i];
    const int o1 = lm_ptr[q + 1];
    int in = 0;
    for (int t = lm_ptr[q]; t < o1; ++t) in |= s.marg[ob[t].y];
    if (in) {
      sel[q] = 1;
      ++n_sel;
    }
  }
  if (n_sel) atomicAdd(&s.n_sel, n_sel);
  __syncthreads();
  if (tid == 0) res->n_marg_pt = s.n_sel;
  if (K == 0) {  // nothing is kept: no output
    if (tid == 0) res->status = 0;
    return;
  }
  double *C6 = d.C6 + pr.m0 * 6, *b3 = d.b3 + pr.m0 * 3;
  double *Ci6 = d.Cinv6 + pr.m0 * 6, *Cib3 = d.Cinvb3 + pr.m0 * 3;
  double *Wg = d.W18 + pr.pair0 * 18;
  // ---- linearise over L, lambda = 0; Schur complement; partial factorisation -------------
  batch_landmark_pass(M, opt_lm, lm_ptr, ob, uvp, s.cams, s.P, X, o.huber, C6, b3, Wg, sel);
  batch_pose_pass(N, d.pobs_ptr + pr.pptr0, d.pobs + pr.pobs0, ob, uvp, s.cams, s.P, X, o.huber, s.A, s.a, sel);
  __syncthreads();
  if (Kp) batch_prior_lin(Kp, pj, pTl, pH, pb, s.P, s.pd, s.pg, s.A, s.a);
  batch_damp_invert(M, 1.0, C6, b3, Ci6, Cib3, opt_lm, sel);
  for (int e = tid; e < nbt * LS; e += kBatchBlock) {  // zero; unit diagonal on the padding of the marked tiles
    const int c = e / LS, r = e - c * LS;
    s.Lb[e] = (r == c && c >= 6 * mp.m && c < 16 * T) ? 1.0 : 0.0;
  }
  __syncthreads();
  batch_schur<nbt, LS, true>(N, M, 1.0, d.tab + pr.tab0, Ci6, Cib3, Wg, s.blk_j, s.blk_k, s.A, s.a, s.Lb, opt_lm,
                             sel, s.col0);
  __syncthreads();
  if (Kp > 1) {
    batch_prior_offdiag<LS, true>(Kp, pj, pH, s.Lb, s.col0);
    __syncthreads();
  }
  chol_lds_partial<NPt, LS>(s.Lb, s.Eb, T, &res->dropped_pivots);  // ends with a barrier
  // ---- the prior: one triangle, mirrored -------------------------------------------------
  double *H = o.H + mp.H_off;
  for (int e = tid; e < K6 * K6; e += kBatchBlock) {
    const int r = e / K6, c = e - r * K6;
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    H[e] = s.Lb[(16 * T + lo) * LS + 16 * T + hi];
  }
  for (int t = tid; t < K6; t += kBatchBlock) o.bvec[mp.b_off + t] = s.Lb[(16 * T + t) * LS + nbt];
  if (tid == 0) res->status = 0;
}

// the widest instances must fit the 160 KiB of LDS a gfx950 workgroup can hold
static_assert(sizeof(BatchLds<6>) <= 160 * 1024, "k_ba_batch<6> exceeds the LDS of a workgroup");
static_assert(sizeof(BatchCovLds<6>) <= 160 * 1024, "k_ba_batch_cov<6> exceeds the LDS of a workgroup");
static_assert(sizeof(BatchMargLds<7>) <= 160 * 1024, "k_ba_batch_marg<7> exceeds the LDS of a workgroup");

}  // namespace
}  // namespace ba

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

size_t lds_bytes_of(int npt) {
  return npt == 2 ? sizeof(ba::BatchLds<2>) : npt == 4 ? sizeof(ba::BatchLds<4>) : sizeof(ba::BatchLds<6>);
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
  if (n_rows > b->rows_cap) {
    if (b->rows) (void)hipFree(b->rows);
    b->rows = nullptr;
    b->rows_cap = 0;
    HIP_TRY(hipMalloc((void **)&b->rows, n_rows * sizeof(ba::DevIterRec)));
    b->rows_cap = n_rows;
  }
  ba::BatchDev d = b->d;
  d.rows = b->rows;
  d.cap = dcap;
  d.lambda0 = (double)opt->initial_lambda;
  d.huber = (double)opt->threshold_huber_loss;
  d.thr_step = (double)opt->threshold_step_size;
  d.thr_cost = (double)opt->threshold_cost_change;
  d.dec_ratio = (double)opt->decrease_ratio_lambda;
  d.inc_ratio = (double)opt->increase_ratio_lambda;
  d.max_iter = opt->max_num_iterations;
  d.gn = opt->gauss_newton ? 1 : 0;
  if (b->npt_class == 2)
    hipLaunchKernelGGL(ba::k_ba_batch<2>, dim3(B), dim3(ba::kBatchBlock), 0, s, d);
  else if (b->npt_class == 4)
    hipLaunchKernelGGL(ba::k_ba_batch<4>, dim3(B), dim3(ba::kBatchBlock), 0, s, d);
  else
    hipLaunchKernelGGL(ba::k_ba_batch<6>, dim3(B), dim3(ba::kBatchBlock), 0, s, d);
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
  if (tiles <= 2)
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
  if (b->npt_class == 2)
    hipLaunchKernelGGL(ba::k_ba_batch_cov<2>, dim3(B), dim3(ba::kBatchBlock), 0, s, b->d, o);
  else if (b->npt_class == 4)
    hipLaunchKernelGGL(ba::k_ba_batch_cov<4>, dim3(B), dim3(ba::kBatchBlock), 0, s, b->d, o);
  else
    hipLaunchKernelGGL(ba::k_ba_batch_cov<6>, dim3(B), dim3(ba::kBatchBlock), 0, s, b->d, o);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(res, o.res, (size_t)B * sizeof(ba_batch_cov_result), hipMemcpyDeviceToHost, s));
  if (b->n_pose > 0)
    HIP_TRY(hipMemcpyAsync(cov_pose36, o.pose36, (size_t)b->n_pose * 36 * sizeof(double), hipMemcpyDeviceToHost, s));
  if (cov_pt9 && b->n_pt > 0)
    HIP_TRY(hipMemcpyAsync(cov_pt9, o.pt9, (size_t)b->n_pt * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
