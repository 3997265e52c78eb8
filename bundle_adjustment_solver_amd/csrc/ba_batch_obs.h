// ba_batch_obs.h — per-observation report, observation mask and outlier cull of the batched
// full bundle adjustment (ba_batch_obs_report, ba_batch_set_obs_mask, ba_batch_cull; DESIGN.md
// §6n).  Three kernels, none of them part of a solve:
//   k_ba_batch_obs_report   one thread per observation of the batch: residual, squared error,
//                           Huber weight and depth at the held values, written in user order
//   k_ba_batch_cull         one workgroup per problem: the cull rule on every on observation,
//                           the starvation rule per optimisable pose, the mask updated in place
//   k_ba_batch_mask_apply   one workgroup per problem: shadow copies of the per-problem lists
//                           (lobs, luv, lm_ptr, pobs, pobs_ptr, BatchProb) without the off
//                           observations, the last-writer bit recomputed among the on ones, W of
//                           pairs left without a writer zeroed
// A masked batch points BatchDev at the shadow lists; k_ba_batch* run what they run today.
// Included by ba_batch.hip only.
#ifndef BA_BATCH_OBS_H_
#define BA_BATCH_OBS_H_
#include "ba_batch_kernels.h"

namespace ba {
namespace {

struct BatchMaskDev {
  const BatchProb *prob;  // the batch as planned (never the shadow)
  const double *cams;
  const double *poses;
  const double *pts;
  const int32_t *jopt;
  const int32_t *opt_lm;
  const int32_t *order;  // per planned observation: its user index (problem-local)
  const int4 *lobs;      // the planned lists
  const double2 *luv;
  const int32_t *lm_ptr, *pair_ptr, *pobs, *pobs_ptr;
  uint8_t *on;      // per observation of the batch, user order: 1 = on
  uint8_t *on_try;  // the cull's candidate mask, same layout
  int32_t *pre;     // per planned observation (+1 per problem): on observations before it
  int4 *lobs_s;     // the shadow lists, at the offsets of the planned ones
  double2 *luv_s;
  int32_t *lm_ptr_s, *pobs_s, *pobs_ptr_s;
  BatchProb *prob_s;
  double *W18;
  ba_batch_cull_result *cres;
};

// exclusive prefix of a flag over the workgroup and its count (every thread calls it)
__device__ __forceinline__ int block_scan_flag(const bool f, int *sm, int &total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long m = __ballot(f);
  const int in_wave = __popcll(m & ((1ull << lane) - 1ull));
  __syncthreads();  // sm is free again
  if (lane == 0) sm[wv] = __popcll(m);
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < kBatchBlock / 64; ++w) {
    const int c = sm[w];
    base += w < wv ? c : 0;
    total += c;
  }
  return base + in_wave;
}

__device__ __forceinline__ int block_sum_int(int v, int *sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < kBatchBlock / 64; ++w) t += sm[w];
  return t;
}

// one observation of problem pr at the held values, from global memory
__device__ __forceinline__ void obs_geom(const BatchMaskDev &m, const BatchProb &pr, const int4 r, const double2 u,
                                         ObsGeom &g) {
  const double *X = m.pts + (size_t)(pr.pt0 + r.z) * 3;
  project(m.cams + (size_t)(pr.cam0 + r.x) * 16, m.poses + (size_t)(pr.pose0 + r.y) * 12, X[0], X[1], X[2], u.x, u.y,
          g);
}

__global__ __launch_bounds__(kBatchBlock) void k_ba_batch_obs_report(const BatchMaskDev m, const int B,
                                                                     const int64_t n_obs, const double huber,
                                                                     double *r2, double *e2, double *w,
                                                                     double *depth) {
  const int64_t t = (int64_t)blockIdx.x * kBatchBlock + threadIdx.x;
  if (t >= n_obs) return;
  int lo = 0, hi = B - 1;  // the last problem whose first observation is not after t
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (m.prob[mid].obs0 <= t) lo = mid; else hi = mid - 1;
  }
  const BatchProb pr = m.prob[lo];
  const int4 r = m.lobs[t];
  ObsGeom g;
  obs_geom(m, pr, r, m.luv[t], g);
  const int64_t k = pr.obs0 + m.order[t];
  if (r2) {
    r2[2 * k] = g.r0;
    r2[2 * k + 1] = g.r1;
  }
  if (e2) e2[k] = g.r0 * g.r0 + g.r1 * g.r1;
  if (w) {
    double wt, G[6];
    weight_and_G(m.cams + (size_t)(pr.cam0 + r.x) * 16, g, huber, wt, G);
    w[k] = wt;
  }
  if (depth) depth[k] = g.Xc[2];
}

__global__ __launch_bounds__(kBatchBlock) void k_ba_batch_cull(const BatchMaskDev m, const double e2_max,
                                                               const int behind) {
  __shared__ int sm[kBatchBlock / 64];
  __shared__ int had[kBatchMaxOpt], has[kBatchMaxOpt];
  const int tid = threadIdx.x;
  const BatchProb pr = m.prob[blockIdx.x];
  ba_batch_cull_result *cr = m.cres + blockIdx.x;
  int bad = pr.status != 0;
  if (!bad) {  // the values k_ba_batch refuses (status 1)
    for (int k = tid; k < pr.n_pose * 12; k += kBatchBlock) bad |= !isfinite(m.poses[pr.pose0 * 12 + k]);
    for (int k = tid; k < pr.n_pt * 3; k += kBatchBlock) bad |= !isfinite(m.pts[pr.pt0 * 3 + k]);
  }
  if (tid < kBatchMaxOpt) had[tid] = has[tid] = 0;
  if (__syncthreads_or(bad)) {
    if (tid == 0) *cr = ba_batch_cull_result{0, 0, 0, pr.status ? pr.status : 1};
    return;
  }
  const int32_t *ord = m.order + pr.obs0;
  uint8_t *on = m.on + pr.obs0, *on_try = m.on_try + pr.obs0;
  int n_before = 0, n_cull = 0;
  for (int t = tid; t < pr.n_obs; t += kBatchBlock) {
    const int k = ord[t];
    int keep = 0;
    if (on[k]) {
      const int4 r = m.lobs[pr.obs0 + t];
      ObsGeom g;
      obs_geom(m, pr, r, m.luv[pr.obs0 + t], g);
      const double e2 = g.r0 * g.r0 + g.r1 * g.r1;
      keep = (e2 <= e2_max) && !(behind && !(g.Xc[2] > 0.0));
      n_before += 1;
      n_cull += !keep;
      const int j = m.jopt[pr.pose0 + r.y];
      if (j >= 0) {  // every writer stores 1
        had[j] = 1;
        if (keep) has[j] = 1;
      }
    }
    on_try[k] = (uint8_t)keep;
  }
  n_before = block_sum_int(n_before, sm);
  n_cull = block_sum_int(n_cull, sm);  // (its barriers also publish had / has)
  int starved = 0;
  for (int j = 0; j < pr.N; ++j) starved |= had[j] && !has[j];
  if (!starved)
    for (int t = tid; t < pr.n_obs; t += kBatchBlock) on[ord[t]] = on_try[ord[t]];
  if (tid == 0) *cr = ba_batch_cull_result{n_before, starved ? 0 : n_cull, starved, 0};
}

__global__ __launch_bounds__(kBatchBlock) void k_ba_batch_mask_apply(const BatchMaskDev m) {
  __shared__ int sm[kBatchBlock / 64];
  __shared__ int start[kBatchMaxOpt + 1];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const BatchProb pr = m.prob[blockIdx.x];
  if (pr.status != 0) {  // never processed: its record only
    if (tid == 0) m.prob_s[blockIdx.x] = pr;
    return;
  }
  const int n = pr.n_obs;
  const int32_t *ord = m.order + pr.obs0;
  const uint8_t *on = m.on + pr.obs0;
  const int4 *ob = m.lobs + pr.obs0;
  int32_t *pre = m.pre + pr.obs0 + blockIdx.x;
  // ---- the compacted position of every observation, in chunks of the workgroup ----------
  int run = 0;
  for (int t0 = 0; t0 < n; t0 += kBatchBlock) {
    const int t = t0 + tid;
    const bool f = t < n && on[ord[t]] != 0;
    int tot;
    const int e = block_scan_flag(f, sm, tot);
    if (t < n) pre[t] = run + e;
    if (f) m.luv_s[pr.obs0 + run + e] = m.luv[pr.obs0 + t];
    run += tot;
  }
  if (tid == 0) pre[n] = run;
  __syncthreads();
  // ---- the records, the last-writer bit among the on observations of a pair -------------
  const int32_t *lp = m.lm_ptr + pr.pt0 + blockIdx.x;
  for (int t = tid; t < n; t += kBatchBlock) {
    if (!on[ord[t]]) continue;
    int4 r = ob[t];
    if (r.w >= 0) {
      const int pid = r.w >> 1, e1 = lp[r.z + 1];
      int later = 0;
      for (int t2 = t + 1; t2 < e1; ++t2) later |= ob[t2].w >= 0 && (ob[t2].w >> 1) == pid && on[ord[t2]] != 0;
      r.w = pid << 1 | (later ? 0 : 1);
    }
    m.lobs_s[pr.obs0 + pre[t]] = r;
  }
  int32_t *lps = m.lm_ptr_s + pr.pt0 + blockIdx.x;
  for (int q = tid; q <= pr.n_pt; q += kBatchBlock) lps[q] = pre[lp[q]];
  // ---- a pair without a writer contributes a zero W: no later kernel writes it ----------
  const int32_t *pair_ptr = m.pair_ptr + pr.m0 + blockIdx.x;
  const int32_t *opt_lm = m.opt_lm + pr.m0;
  for (int i = tid; i < pr.M; i += kBatchBlock) {
    const int q = opt_lm[i], o0 = lp[q], o1 = lp[q + 1];
    for (int p = pair_ptr[i]; p < pair_ptr[i + 1]; ++p) {
      int writer = 0;
      for (int t = o0; t < o1; ++t) writer |= ob[t].w >= 0 && (ob[t].w >> 1) == p && on[ord[t]] != 0;
      if (!writer) {
        double *W = m.W18 + (size_t)(pr.pair0 + p) * 18;
        for (int e = 0; e < 18; ++e) W[e] = 0.0;
      }
    }
  }
  // ---- the pose-major list: one wave per optimisable pose, counts first ----------------
  const int32_t *pp = m.pobs_ptr + pr.pptr0, *po = m.pobs + pr.pobs0;
  for (int j = wv; j < pr.N; j += kBatchBlock / 64) {
    int c = 0;
    const int e1 = pp[j + 1];
    for (int t0 = pp[j]; t0 < e1; t0 += 64) {
      const int t = t0 + lane;
      c += __popcll(__ballot(t < e1 && on[ord[po[t < e1 ? t : t0]]] != 0));
    }
    if (lane == 0) start[j + 1] = c;
  }
  __syncthreads();
  if (tid == 0) {
    start[0] = 0;
    for (int j = 0; j < pr.N; ++j) start[j + 1] += start[j];
  }
  __syncthreads();
  for (int j = tid; j <= pr.N; j += kBatchBlock) m.pobs_ptr_s[pr.pptr0 + j] = start[j];
  for (int j = wv; j < pr.N; j += kBatchBlock / 64) {
    int at = start[j];
    const int e1 = pp[j + 1];
    for (int t0 = pp[j]; t0 < e1; t0 += 64) {
      const int t = t0 + lane;
      const int so = po[t < e1 ? t : t0];
      const bool f = t < e1 && on[ord[so]] != 0;
      const unsigned long long bm = __ballot(f);
      if (f) m.pobs_s[pr.pobs0 + at + __popcll(bm & ((1ull << lane) - 1ull))] = pre[so];
      at += __popcll(bm);
    }
  }
  if (tid == 0) {
    BatchProb ps = pr;
    ps.n_obs = run;
    m.prob_s[blockIdx.x] = ps;
  }
}

}  // namespace
}  // namespace ba
#endif  // BA_BATCH_OBS_H_
