// ba_batch_kernels.h — the device side of the batched full bundle adjustment: the structures
// the host fills, the steps shared by the three kernels and the kernels themselves
// (k_ba_batch, k_ba_batch_cov, k_ba_batch_marg).  Included by ba_batch.hip, which compiles the
// instances without relative-pose factors and holds the host side, and by ba_batch_rel.hip,
// which compiles the instances with them; see ba_batch.hip for the description.
#ifndef BA_BATCH_KERNELS_H_
#define BA_BATCH_KERNELS_H_
#include <hip/hip_runtime.h>

#include "ba_chol_lds.h"
#include "ba_device_fn.h"
#include "ba_handle.h"
#include "ba_rel_fn.h"

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

// the relative-pose factors of one problem (ba_batch_set_relative): element offsets into the
// factor arrays; F = 0: none
struct BatchRel {
  int64_t f0;        // first factor
  int64_t pp0, pl0;  // per optimisable pose: N + 1 pointers, list entries
  int64_t b0, bp0, bl0;  // coupled blocks: records, nblk + 1 pointers, list entries
  int32_t F, nblk;
};

// the arrays of the relative-pose factors (ba_batch_set_relative), one record on the device;
// a pointer to it is the last argument of the REL instances of the kernels, which no other
// instance takes (ten pointers among the kernel arguments cost k_ba_batch<4> scalar spills)
struct BatchRelDev {
  const BatchRel *rel;    // per problem
  const int4 *rel_jk;     // per factor: {pose j, pose k, optimisable index of j or -1, of k or -1}
  const double *rel_Z, *rel_Om;
  const int32_t *rel_pptr, *rel_plist, *rel_bptr, *rel_blist;
  const int2 *rel_blk;
  double *rel_scr;        // kRelScr doubles per factor
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

// ---- the relative-pose factors of one problem, shared by the three kernels ----------------
// The factor itself is ba_rel_fn.h's; here is what belongs to a batch.  Unlike the prior's H
// the factor's blocks depend on the poses, so they are rebuilt per linearisation into the
// problem's slice of global scratch
// (kRelScr doubles per factor, nothing in LDS) and then gathered by one thread per element
// of A_j, a_j and of every coupled block, each walking its list in input order.
// on (here and below): nullptr, or one byte per pose of the problem; a factor joins when one
// of its two poses is marked (k_ba_batch_marg)
struct RelView {
  int F, N, nblk;
  const int4 *jk;         // per factor: {pose j, pose k, optimisable index of j or -1, of k or -1}
  const double *Z, *Om;   // 12 and 36 (symmetric, mirrored by the host) per factor
  const int32_t *pptr, *plist;  // per optimisable pose: factor << 1 | (1: it is the factor's k)
  const int2 *blk;              // per coupled block: optimisable poses {hi, lo}, hi > lo
  const int32_t *bptr, *blist;  // per coupled block: factor << 1 | (1: H_jk lies transposed)
  double *scr;
};

// the view is built where it is used, from the kernel argument and the problem's record: the
// kernels keep only the two counts of the record across their other steps
__device__ __forceinline__ RelView rel_view(const BatchRelDev &d, const int N) {
  const BatchRel rr = d.rel[blockIdx.x];
  RelView v;
  v.F = rr.F;
  v.N = N;
  v.nblk = rr.nblk;
  v.jk = d.rel_jk + rr.f0;
  v.Z = d.rel_Z + rr.f0 * 12;
  v.Om = d.rel_Om + rr.f0 * 36;
  v.pptr = d.rel_pptr + rr.pp0;
  v.plist = d.rel_plist + rr.pl0;
  v.blk = d.rel_blk + rr.b0;
  v.bptr = d.rel_bptr + rr.bp0;
  v.blist = d.rel_blist + rr.bl0;
  v.scr = d.rel_scr + rr.f0 * kRelScr;
  return v;
}

// the two counts of the problem's record (uniform per workgroup); 0: no factors, no coupled block
__device__ __forceinline__ int rel_factors(const BatchRelDev &d) { return d.rel[blockIdx.x].F; }
__device__ __forceinline__ int rel_blocks(const BatchRelDev &d) { return d.rel[blockIdx.x].nblk; }
// the factor arrays among the arguments of a REL instance
__device__ __forceinline__ const BatchRelDev &rel_arg(const BatchRelDev *r) { return *r; }

__device__ __forceinline__ bool rel_on(const int4 jk, const uint8_t *on) { return !on || on[jk.x] || on[jk.y]; }
struct RelOff {  // the skip predicate of the two list walks
  const int4 *jk;
  const uint8_t *on;
  __device__ __forceinline__ bool operator()(int f) const { return !rel_on(jk[f], on); }
};

// Part 1, after batch_pose_pass (and the prior's part 1): the blocks of every factor into
// the scratch, then Omega / Ad^T Omega Ad into A_j / A_k and -Omega r / Ad^T Omega r into
// a_j / a_k: the diagonal is damped with the rest of A_j.  Ends with a barrier.
__device__ __forceinline__ void batch_rel_lin(const BatchRelDev &d, const int N, const double *P, double *A, double *a,
                                              const uint8_t *on = nullptr) {
  const RelView v = rel_view(d, N);
  const int tid = threadIdx.x;
  // r and Ad, one thread per factor
  for (int f = tid; f < v.F; f += kBatchBlock) {
    const int4 jk = v.jk[f];
    if (!rel_on(jk, on)) continue;
    double RE[9], tE[3];
    rel_E(jk, P, RE, tE);
    double *s = v.scr + (size_t)f * kRelScr;
    rel_Ad(RE, tE, s + kRelAd);
    rel_log(RE, tE, v.Z + (size_t)f * 12, s + kRelR);
  }
  __syncthreads();
  // OA = Omega Ad and Or = Omega r, one thread per element
  for (int e = tid; e < 42 * v.F; e += kBatchBlock) {
    const int f = e / 42, q = e - 42 * f;
    if (!rel_on(v.jk[f], on)) continue;
    const double *Om = v.Om + (size_t)f * 36;
    double *s = v.scr + (size_t)f * kRelScr;
    if (q < 36)
      s[kRelOA + q] = factor_OA<6>(Om, s + kRelAd, q);
    else
      s[kRelOr + q - 36] = factor_Or<6>(Om, s + kRelR, q - 36);
  }
  __syncthreads();
  // Bk = Ad^T OA and gk = Ad^T Or, one thread per element
  for (int e = tid; e < 42 * v.F; e += kBatchBlock) {
    const int f = e / 42, q = e - 42 * f;
    const int4 jk = v.jk[f];
    if (jk.w < 0 || !rel_on(jk, on)) continue;
    double *s = v.scr + (size_t)f * kRelScr;
    if (q < 36)
      s[kRelBk + q] = factor_Bk<6>(s + kRelAd, s + kRelOA, q);
    else
      s[kRelGk + q - 36] = factor_gk<6>(s + kRelAd, s + kRelOr, q - 36);
  }
  __syncthreads();
  // gather: one thread per element of A_j and a_j, the pose's factors in input order
  for (int e = tid; e < 42 * v.N; e += kBatchBlock) {
    const int j = e / 42, q = e - 42 * j;
    bool any = false;
    const double acc = rel_walk_pose(v.Om, 36, v.scr, v.plist, v.pptr[j], v.pptr[j + 1], q, RelOff{v.jk, on}, &any);
    if (!any) continue;  // a pose without a joining factor keeps its bits (and its exact zeros)
    if (q < 36)
      A[j * 36 + q] += acc;
    else
      a[j * 6 + q - 36] += acc;
  }
  __syncthreads();
}

// Part 2, after batch_schur (and the prior's part 2) and a barrier: H_jk = -Omega Ad of every
// coupled block, undamped, into the lower triangle of the image; one thread per element,
// the block's factors in input order.  PERM as in batch_prior_offdiag.  The blocks are read
// from the scratch, so after a SKIPPED step the same bits go back into the reset image.
template <int LS, bool PERM>
__device__ __forceinline__ void batch_rel_offdiag(const BatchRelDev &d, const int N, double *Lb,
                                                  const uint8_t *col0 = nullptr, const uint8_t *on = nullptr) {
  const RelView v = rel_view(d, N);
  for (int e = threadIdx.x; e < 36 * v.nblk; e += kBatchBlock) {
    const int b = e / 36, rc = e - 36 * b, r = rc / 6, c = rc - 6 * r;
    const int2 hl = v.blk[b];
    bool any = false;
    const double acc = rel_walk_block(v.scr, v.blist, v.bptr[b], v.bptr[b + 1], r, c, RelOff{v.jk, on}, &any);
    if (!any) continue;
    const int row = (PERM ? col0[hl.x] : 6 * hl.x) + r, col = (PERM ? col0[hl.y] : 6 * hl.y) + c;
    Lb[PERM && row < col ? row * LS + col : col * LS + row] += acc;
  }
}

// sum over the factors of sqrt(max(0, r^T Omega r)) at the poses P: one residual per factor,
// its norm added as an observation's is; one thread per factor, one block_sum; thread 0
__device__ __forceinline__ double batch_rel_cost(const BatchRelDev &d, const int N, const double *P, double *red) {
  const RelView v = rel_view(d, N);
  double acc = 0.0;
  for (int f = threadIdx.x; f < v.F; f += kBatchBlock) {
    double RE[9], tE[3], r[6];
    rel_E(v.jk[f], P, RE, tE);
    rel_log(RE, tE, v.Z + (size_t)f * 12, r);
    acc += sqrt(fmax(0.0, factor_quad<6>(v.Om + (size_t)f * 36, r)));
  }
  return block_sum(acc, red);
}

// the cross term 2 sum_f x_j^T H_jk x_k of the quadratic model over the factors with two
// optimisable poses, one factor per thread
__device__ __forceinline__ double batch_rel_cross(const BatchRelDev &d, const int N, const double *xs) {
  const RelView v = rel_view(d, N);
  double est = 0.0;
  for (int f = threadIdx.x; f < v.F; f += kBatchBlock) {
    const int4 jk = v.jk[f];
    if (jk.z < 0 || jk.w < 0) continue;
    est += rel_cross(v.scr + (size_t)f * kRelScr + kRelOA, xs + 6 * jk.z, xs + 6 * jk.w);
  }
  return est;
}

// REL (here and in the other two kernels): the batch has relative-pose factors set; the
// instance then takes their arrays as one more argument (R = const BatchRelDev *).  The REL = false
// instances take no such argument, hold none of that code and are compiled in ba_batch.hip
// as before; the REL instances are compiled in ba_batch_rel.hip, a code object of their own.
// The host picks the instance per launch.
template <int NPt, bool REL, class... R>
__global__ __launch_bounds__(kBatchBlock) void k_ba_batch(BatchDev d, R... rel) {
  static_assert(sizeof...(R) == (REL ? 1 : 0), "a REL instance takes the factor arrays, no other does");
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
  // the relative-pose factors of this problem (uniform per workgroup); Fr = 0: none
  int Fr = 0, Br = 0;
  if constexpr (REL) {
    Fr = rel_factors(rel_arg(rel...));
    Br = rel_blocks(rel_arg(rel...));
  }
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
    if constexpr (REL) if (Fr) {
      const double rc = batch_rel_cost(rel_arg(rel...), N, s.P[0], s.red);
      c0 += rc;
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
      if constexpr (REL) if (Fr) batch_rel_lin(rel_arg(rel...), N, Pc, s.A, s.a);
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
    if constexpr (REL) if (Br) {
      batch_rel_offdiag<LS, false>(rel_arg(rel...), N, s.Lb);
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
    if constexpr (REL) if (Br) estp += batch_rel_cross(rel_arg(rel...), N, s.xs);
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
    if constexpr (REL) if (Fr) {
      const double rc = batch_rel_cost(rel_arg(rel...), N, Pt, s.red);
      tc += rc;
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
template <int NPt, bool REL, class... R>
__global__ __launch_bounds__(kBatchBlock) void k_ba_batch_cov(BatchDev d, BatchCovOut o, R... rel) {
  static_assert(sizeof...(R) == (REL ? 1 : 0), "a REL instance takes the factor arrays, no other does");
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
  if constexpr (REL) if (rel_factors(rel_arg(rel...))) batch_rel_lin(rel_arg(rel...), N, s.P, s.A, s.a);
  batch_damp_invert(M, 1.0, C6, b3, Ci6, Cib3);
  batch_reset_image<nbt, LS>(s.Lb, n6);
  __syncthreads();
  batch_schur<nbt, LS>(N, M, 1.0, d.tab + pr.tab0, Ci6, Cib3, Wg, s.blk_j, s.blk_k, s.A, s.a, s.Lb);
  __syncthreads();
  if (Kp > 1) {
    batch_prior_offdiag<LS, false>(Kp, pj, pH, s.Lb);
    __syncthreads();
  }
  if constexpr (REL) if (rel_blocks(rel_arg(rel...))) {
    batch_rel_offdiag<LS, false>(rel_arg(rel...), N, s.Lb);
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
template <int NPt, bool REL, class... R>
__device__ __forceinline__ void batch_marg_body(const BatchDev &d, const BatchMargOut &o, const R &...rel) {
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
  if constexpr (REL) if (rel_factors(rel_arg(rel...))) batch_rel_lin(rel_arg(rel...), N, s.P, s.A, s.a, s.marg);  // a factor joins when one of its poses is marked
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
  if constexpr (REL) if (rel_blocks(rel_arg(rel...))) {
    batch_rel_offdiag<LS, true>(rel_arg(rel...), N, s.Lb, s.col0, s.marg);
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

template <int NPt>
__global__ __launch_bounds__(kBatchBlock) void k_ba_batch_marg(BatchDev d, BatchMargOut o) {
  batch_marg_body<NPt, false>(d, o);
}

// With the factors: the 32-column instance ran three waves per SIMD on 166 of the 168
// registers that allows and needs a few more with this code; the hint keeps it at three waves
// (160 VGPRs, no AGPR).  The wider instances are bounded by their LDS.  The kernel without
// factors above carries no hint and is allocated as it always was.
template <int NPt>
__global__ __launch_bounds__(kBatchBlock) __attribute__((amdgpu_waves_per_eu(NPt == 2 ? 3 : 1))) void k_ba_batch_marg_rel(
    BatchDev d, BatchMargOut o, const BatchRelDev *rel) {
  batch_marg_body<NPt, true>(d, o, rel);
}

// the widest instances must fit the 160 KiB of LDS a gfx950 workgroup can hold
static_assert(sizeof(BatchLds<6>) <= 160 * 1024, "k_ba_batch<6> exceeds the LDS of a workgroup");
static_assert(sizeof(BatchCovLds<6>) <= 160 * 1024, "k_ba_batch_cov<6> exceeds the LDS of a workgroup");
static_assert(sizeof(BatchMargLds<7>) <= 160 * 1024, "k_ba_batch_marg<7> exceeds the LDS of a workgroup");

}  // namespace
}  // namespace ba

namespace ba {
// Launch of the REL instance of one kernel (ba_batch_rel.hip), one workgroup per problem:
// kernel 0 = k_ba_batch, 1 = k_ba_batch_cov, 2 = k_ba_batch_marg_rel; npt = 16-column panels
// of the image; dev / out / rel point to the BatchDev, the BatchCovOut or BatchMargOut (kernel
// 0: unused) of the launch, rel is the device address of the BatchRelDev.  The structures live in an unnamed namespace
// of this header, hence the untyped pointers.
void batch_launch_rel(int kernel, int npt, int B, hipStream_t s, const void *dev, const void *out, const void *rel);
}  // namespace ba
#endif  // BA_BATCH_KERNELS_H_
