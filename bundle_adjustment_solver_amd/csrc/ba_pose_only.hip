// ba_pose_only.hip — pose-only Gauss-Newton, 6-DoF and planar 3-DoF (monocular
// and stereo), fp32, gfx950.
//
// Replaces PoseOnlyBundleAdjustmentSolver::Solve_Monocular_6Dof (reference
// core/pose_only_bundle_adjustment_solver.cpp:8-170 with helpers :1338-1452,
// :1147-1200, :1280-1316) and ::Solve_Stereo_6Dof (:172-399: the right camera
// sees X_r = left_to_right^-1 * X_l, contributes where its pixel is
// non-negative, has its own inlier mask; the error is normalised by
// (count_left + count_right) * 0.5f).  The whole GN loop runs inside ONE persistent
// launch of up to 64 co-resident workgroups (the problem is 10 k points ~ 200 KB:
// launch / PCIe latency dominates, not bandwidth): per iteration every thread
// linearises its points, the 21+6+1+1 sums are reduced through DPP + LDS and,
// across workgroups, through one grid barrier; thread 0 of every workgroup solves
// the 6x6 system with the pivoted LDL^T the reference gets from Eigen and
// composes the se3 exponential onto the pose held in LDS.
//
// k_pose_only3 replaces ::Solve_Monocular_Planar3Dof / ::Solve_Stereo_Planar3Dof
// (:401-900, helpers :1202-1278, :1454-1583) in the same shape: 6+3+1+1 sums,
// a 3x3 pivoted LDL^T, and the reference's left-multiplicative (x, y, psi) update.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/ba_hip.h"
#include "ba_device.h"

namespace ba {

namespace {

constexpr int kPoThreads = 1024;
constexpr int kPoWaves = kPoThreads / 64;
constexpr int kPoMaxGroups = 64;   // workgroups of one launch (all co-resident)
constexpr int kPoPointsPerThread = 2;  // aimed at when choosing the group count
constexpr int kNred = 29;  // 21 upper H + 6 g + 1 err + 1 count of right-camera edges

// Wave-wide fp32 sum on the DPP network (xor-1, xor-2, half-mirror, mirror leave
// every lane with the total of its row of 16; the four row totals are added in
// order).  Fixed association; every lane returns the total.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_f32(float v, int src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}
__device__ __forceinline__ float wave_sum_f(float v) {
  v += dpp_f32<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f32<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f32<0x141>(v);  // row_half_mirror
  v += dpp_f32<0x140>(v);  // row_mirror
  return ((lane_f32(v, 0) + lane_f32(v, 16)) + lane_f32(v, 32)) + lane_f32(v, 48);
}

// Eigen-style pivoted LDL^T solve of an NxN system in fp32 (thread 0 only;
// N = 6 for k_pose_only6, N = 3 for k_pose_only3).
// m, d, tr, tmp point to LDS: the pivoted algorithm indexes them dynamically,
// which would otherwise put them in scratch (global) memory.
template <int N>
__device__ void ldlt_solve(float *m /*N*N, row-major, lower used*/, float *d, int *tr,
                           float *tmp) {
#define AT(r, c) m[(r) * N + (c)]
  bool early = false;
  for (int k = 0; k < N && !early; ++k) {
    int big = k;
    float bigv = fabsf(AT(k, k));
    for (int i = k + 1; i < N; ++i)
      if (fabsf(AT(i, i)) > bigv) {
        bigv = fabsf(AT(i, i));
        big = i;
      }
    tr[k] = big;
    if (k != big) {
      const int s = N - big - 1;
      for (int c = 0; c < k; ++c) {
        float t = AT(k, c); AT(k, c) = AT(big, c); AT(big, c) = t;
      }
      for (int r = 0; r < s; ++r) {
        float t = AT(big + 1 + r, k);
        AT(big + 1 + r, k) = AT(big + 1 + r, big);
        AT(big + 1 + r, big) = t;
      }
      {
        float t = AT(k, k); AT(k, k) = AT(big, big); AT(big, big) = t;
      }
      for (int i = k + 1; i < big; ++i) {
        float t = AT(i, k); AT(i, k) = AT(big, i); AT(big, i) = t;
      }
    }
    const int rs = N - k - 1;
    if (k > 0) {
      float acc = 0.0f;
      for (int c = 0; c < k; ++c) {
        tmp[c] = AT(c, c) * AT(k, c);
        acc += AT(k, c) * tmp[c];
      }
      AT(k, k) -= acc;
      for (int r = 0; r < rs; ++r) {
        float s2 = 0.0f;
        for (int c = 0; c < k; ++c) s2 += AT(k + 1 + r, c) * tmp[c];
        AT(k + 1 + r, k) -= s2;
      }
    }
    const float akk = AT(k, k);
    const bool valid = fabsf(akk) > 0.0f;
    if (k == 0 && !valid) {
      for (int j = 0; j < N; ++j) tr[j] = j;
      early = true;
      break;
    }
    if (rs > 0 && valid)
      for (int r = 0; r < rs; ++r) AT(k + 1 + r, k) /= akk;
  }
  for (int i = 0; i < N; ++i)
    if (tr[i] != i) { float t = d[i]; d[i] = d[tr[i]]; d[tr[i]] = t; }
  for (int i = 0; i < N; ++i) {
    float s = d[i];
    for (int c = 0; c < i; ++c) s -= AT(i, c) * d[c];
    d[i] = s;
  }
  for (int i = 0; i < N; ++i) {
    if (fabsf(AT(i, i)) > 1.17549435e-38f) d[i] /= AT(i, i);
    else d[i] = 0.0f;
  }
  for (int i = N - 1; i >= 0; --i) {
    float s = d[i];
    for (int r = i + 1; r < N; ++r) s -= AT(r, i) * d[r];
    d[i] = s;
  }
  for (int i = N - 1; i >= 0; --i)
    if (tr[i] != i) { float t = d[i]; d[i] = d[tr[i]]; d[tr[i]] = t; }
#undef AT
}

// One camera's terms of one point (reference :1350-1452) added to acc.
__device__ __forceinline__ void po_edge(const float Lp[3], float fx, float fy, float cx,
                                        float cy, float pu, float pv, float thr_huber,
                                        float thr_out, float acc[kNred], uint8_t *mk) {
  // reference :1350-1384
  const float iz = 1.0f / Lp[2];
  const float xiz = Lp[0] * iz, yiz = Lp[1] * iz;
  const float fxxiz = fx * xiz, fyyiz = fy * yiz;
  const float ru = (fxxiz + cx) - pu;
  const float rv = (fyyiz + cy) - pv;
  float Ju[6], Jv[6];
  Ju[0] = fx * iz; Ju[1] = 0.0f; Ju[2] = -fxxiz * iz; Ju[3] = -fxxiz * yiz;
  Ju[4] = fx * (1.0f + xiz * xiz); Ju[5] = -fx * yiz;
  Jv[0] = 0.0f; Jv[1] = fy * iz; Jv[2] = -fyyiz * iz;
  Jv[3] = -fy * (1.0f + yiz * yiz); Jv[4] = fyyiz * xiz; Jv[5] = fy * xiz;
  // reference :1386-1452
  const float ars = fabsf(ru) + fabsf(rv);
  const bool hub = ars >= thr_huber;
  const float w = hub ? thr_huber / ars : 1.0f;
  const float wru = hub ? w * ru : ru, wrv = hub ? w * rv : rv;
  // per-edge Hessian first, then added to the running sums (the reference forms
  // hessian_i and appends it: same association)
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) {
      float hv = 0.0f;
      if (r != 1 && c != 1) hv += hub ? (w * Ju[r]) * Ju[c] : Ju[r] * Ju[c];
      if (r != 0 && c != 0) hv += hub ? (w * Jv[r]) * Jv[c] : Jv[r] * Jv[c];
      acc[k++] += hv;
    }
#pragma unroll
  for (int c = 0; c < 6; ++c) acc[21 + c] -= wru * Ju[c] + wrv * Jv[c];
  acc[27] += hub ? wru * ru : rv * rv;  // reference :1432,:1450 (Q9)
  if (ars >= thr_out) *mk = 0;          // reference :95-98 / :287-290, :321-324
}

// meta[0] = iterations executed, meta[1] = converged, meta[2] = rows logged,
// meta[3] = success (0 = NaN)
// STEREO: uvr2 = right pixels, cam_r = {fx,fy,cx,cy, Rrl(9), trl(3)} with
// (Rrl, trl) = left_to_right^-1, maskr = right inlier mask.
// Grid-wide barrier of the co-resident workgroups of ONE launch (gridDim.x <=
// kPoMaxGroups workgroups of 1024 threads always fit the 256 CUs at once).
// gsync[0] counts arrivals, monotonically: barrier number b is passed when it
// reaches (b+1)*gridDim.x.  The release add publishes this workgroup's partial
// sums, the acquire load makes the others' visible (and invalidates the CU's
// L1 for every wave of the workgroup).  The spin is bounded: on a time-out
// gsync[1] is set and the kernel still runs to its end, so the grid always
// drains; the host then reports an error.
__device__ __forceinline__ void po_grid_barrier(int *gsync, int target) {
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(&gsync[0], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    int spins = 0;
    while (__hip_atomic_load(&gsync[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < target) {
      if (++spins > (1 << 22)) {
        gsync[1] = 1;
        break;
      }
      __builtin_amdgcn_s_sleep(4);
    }
  }
  __syncthreads();
}

// Several workgroups (one per CU) share the points of one problem: each
// linearises its share, the 29 partial sums meet in `partial` (double-buffered
// by iteration parity), ONE grid barrier per Gauss-Newton iteration, and then
// EVERY workgroup adds the partials in the same order and runs the same 6x6
// solve, so all hold the same pose and take the same convergence decision
// without a second barrier or a broadcast.  Workgroup 0 writes the outputs.
//
// BATCH (ba_pose_only_{mono,stereo}6_batch): B independent problems, one
// workgroup each, launched with B workgroups.  The arguments are then per-batch
// arrays, re-pointed at problem b = blockIdx.x on entry: gsync = offsets (B+1;
// the problem's points are [offsets[b], offsets[b+1])), partial = intrinsics
// (B x 4), cam_r = right-camera records (B x 16), T12 (B x 12), iters (B x cap),
// debug_T12 (B x cap x 12), meta = ba_po_result records (B x 4 ints: status 0 =
// pose written, 1 = NaN, 2 = empty range and nothing else written); n and
// fx..cy are unused.  G = 1 and block 0 at compile time: no exchange, no grid
// barrier, no workgroup waits for another (any B is safe), and the arithmetic is
// that of a one-workgroup launch of k_pose_only6<STEREO, false>.
template <bool STEREO, bool BATCH>
__global__ __launch_bounds__(kPoThreads) void k_pose_only6(
    const float *__restrict__ X3, const float *__restrict__ uv2,
    const float *__restrict__ uvr2, int n, float fx, float fy, float cx, float cy,
    const float *__restrict__ cam_r, float *T12, uint8_t *mask, uint8_t *maskr,
    float thr_huber, float thr_step, float thr_cost, float thr_out, int max_it,
    PoIter *iters, int cap, int *meta, float *debug_T12, int *gsync, float *partial) {
  if constexpr (BATCH) {
    const unsigned b = blockIdx.x;
    const int o = gsync[b];
    n = gsync[b + 1] - o;
    meta += 4 * (size_t)b;
    if (n <= 0) {
      if (threadIdx.x == 0) {
        meta[0] = 0;
        meta[1] = 0;
        meta[2] = 0;
        meta[3] = 2;
      }
      return;
    }
    X3 += 3 * (size_t)o;
    uv2 += 2 * (size_t)o;
    mask += o;
    if (STEREO) {
      uvr2 += 2 * (size_t)o;
      maskr += o;
      cam_r += 16 * (size_t)b;
    }
    fx = partial[4 * b];
    fy = partial[4 * b + 1];
    cx = partial[4 * b + 2];
    cy = partial[4 * b + 3];
    T12 += 12 * (size_t)b;
    if (iters) iters += (size_t)b * cap;
    if (debug_T12) debug_T12 += (size_t)b * cap * 12;
  }
  const int G = BATCH ? 1 : gridDim.x;
  const bool lead = BATCH ? true : blockIdx.x == 0;
  __shared__ float red[kPoWaves][kNred];
  __shared__ float tots[kNred];
  __shared__ float Hs[36], gs[6], tmps[6];
  __shared__ int trs[6];
  __shared__ float pose[12];  // camera_to_world_optimized: R (9) then t (3)
  __shared__ int ctl[2];      // [0] = stop flag
  __shared__ float s_err_prev;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) {
    // pose = reference_to_current.inverse()  (reference :52-53)
    float R[9];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) R[r * 3 + c] = T12[c * 3 + r];
    for (int k = 0; k < 9; ++k) pose[k] = R[k];
    for (int r = 0; r < 3; ++r)
      pose[9 + r] = -(R[r * 3 + 0] * T12[9] + R[r * 3 + 1] * T12[10] +
                      R[r * 3 + 2] * T12[11]);
    ctl[0] = 0;
    ctl[1] = 0;  // iterations executed
    s_err_prev = 1e10f;
    if (lead) {
      meta[0] = 0;
      meta[1] = 1;
      meta[2] = 0;
      meta[3] = BATCH ? 0 : 1;
    }
  }
  int n_rows = 0;  // Summary rows logged so far (thread 0)
  __syncthreads();
  const float inv_n = 1.0f / (float)n;
  for (int it = 0; it < max_it; ++it) {
    float Rl[9], tl[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rl[k] = pose[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tl[k] = pose[9 + k];
    float acc[kNred];
#pragma unroll
    for (int k = 0; k < kNred; ++k) acc[k] = 0.0f;
    float cr[16];
    if (STEREO) {
#pragma unroll
      for (int k = 0; k < 16; ++k) cr[k] = cam_r[k];
    }
    // four points per trip: their loads are issued together, so a trip pays one
    // memory latency instead of four (the inputs are re-read from L2 in every
    // Gauss-Newton iteration)
    const int gstride = G * kPoThreads;
    for (int p0 = (BATCH ? 0u : blockIdx.x) * kPoThreads + tid; p0 < n; p0 += 4 * gstride) {
      float Xb[4][3], ub[4][2], urb[4][2];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + u * gstride;
        const int pc = p < n ? p : n - 1;
        Xb[u][0] = X3[3 * pc]; Xb[u][1] = X3[3 * pc + 1]; Xb[u][2] = X3[3 * pc + 2];
        ub[u][0] = uv2[2 * pc]; ub[u][1] = uv2[2 * pc + 1];
        if (STEREO) { urb[u][0] = uvr2[2 * pc]; urb[u][1] = uvr2[2 * pc + 1]; }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + u * gstride;
        if (p >= n) break;
        float Lp[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
          Lp[r] = (Rl[r * 3 + 0] * Xb[u][0] + Rl[r * 3 + 1] * Xb[u][1] + Rl[r * 3 + 2] * Xb[u][2]) + tl[r];
        po_edge(Lp, fx, fy, cx, cy, ub[u][0], ub[u][1], thr_huber, thr_out, acc, mask + p);
        if (STEREO) {
          const float pu = urb[u][0], pv = urb[u][1];
          if (!(pu < 0 || pv < 0)) {  // reference :298
            float Lr[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
              Lr[r] = (cr[4 + r * 3 + 0] * Lp[0] + cr[4 + r * 3 + 1] * Lp[1] +
                       cr[4 + r * 3 + 2] * Lp[2]) +
                      cr[13 + r];
            po_edge(Lr, cr[0], cr[1], cr[2], cr[3], pu, pv, thr_huber, thr_out, acc, maskr + p);
            acc[28] += 1.0f;
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kNred; ++k) {
      const float s = wave_sum_f(acc[k]);
      if (lane == 0) red[wv][k] = s;
    }
    __syncthreads();
    // cross-wave sums in parallel (thread k adds the 16 wave totals of sum k in
    // order), then thread 0 runs the 6x6 solve
    if (tid < kNred) {
      float sk = 0.0f;
#pragma unroll
      for (int w = 0; w < kPoWaves; ++w) sk += red[w][tid];
      tots[tid] = sk;
    }
    if (G > 1) {
      float *pb = partial + (size_t)(it & 1) * kPoMaxGroups * kNred;
      // agent-scope accesses: the partials cross XCDs (separate L2s)
      if (tid < kNred)
        __hip_atomic_store(&pb[blockIdx.x * kNred + tid], tots[tid], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      po_grid_barrier(gsync, (it + 1) * G);
      if (tid < kNred) {  // every workgroup: the same sum in the same order
        float sk = 0.0f;
        for (int w = 0; w < G; ++w)
          sk += __hip_atomic_load(&pb[w * kNred + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tots[tid] = sk;
      }
    }
    __syncthreads();
    if (tid == 0) {
      float tot[kNred];
#pragma unroll
      for (int k = 0; k < kNred; ++k) tot[k] = tots[k];
      float *H = Hs, *g = gs;
      int k = 0;
      for (int r = 0; r < 6; ++r)
        for (int c = r; c < 6; ++c) {
          H[r * 6 + c] = tot[k];
          H[c * 6 + r] = tot[k];
          ++k;
        }
      for (int r = 0; r < 6; ++r) H[r * 6 + r] *= (1.0f + 1e-5f);  // :103
      for (int c = 0; c < 6; ++c) g[c] = tot[21 + c];
      ldlt_solve<6>(H, g, trs, tmps);  // delta_xi, reference :105
      // se3 exponential, reference :1280-1316
      const float v0 = g[0], v1 = g[1], v2 = g[2], w0 = g[3], w1 = g[4], w2 = g[5];
      const float theta = sqrtf(w0 * w0 + w1 * w1 + w2 * w2);
      const float wx[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
      float wx2[9];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
          wx2[r * 3 + c] = wx[r * 3 + 0] * wx[0 * 3 + c] + wx[r * 3 + 1] * wx[1 * 3 + c] +
                           wx[r * 3 + 2] * wx[2 * 3 + c];
      float ca, cb, va, vb;
      if (theta < 1e-7f) {
        ca = 1.0f; cb = 0.5f; va = 0.5f; vb = 0.33333333333333333333333333f;
      } else {
        const float st = sinf(theta), ct = cosf(theta);
        ca = st / theta;
        cb = (1.0f - ct) / (theta * theta);
        va = cb;
        vb = (theta - st) / (theta * theta * theta);
      }
      float dR[9], V[9], dt[3];
      for (int q = 0; q < 9; ++q) {
        const float id = (q % 4 == 0) ? 1.0f : 0.0f;
        dR[q] = id + ca * wx[q] + cb * wx2[q];
        V[q] = id + va * wx[q] + vb * wx2[q];
      }
      for (int r = 0; r < 3; ++r) dt[r] = V[r * 3 + 0] * v0 + V[r * 3 + 1] * v1 + V[r * 3 + 2] * v2;
      float Rn[9], tn[3];
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
          Rn[r * 3 + c] = dR[r * 3 + 0] * pose[0 * 3 + c] + dR[r * 3 + 1] * pose[1 * 3 + c] +
                          dR[r * 3 + 2] * pose[2 * 3 + c];
        tn[r] = dR[r * 3 + 0] * pose[9] + dR[r * 3 + 1] * pose[10] + dR[r * 3 + 2] * pose[11] + dt[r];
      }
      for (int q = 0; q < 9; ++q) pose[q] = Rn[q];
      for (int q = 0; q < 3; ++q) pose[9 + q] = tn[q];
      if (lead && debug_T12 && it < cap) {
        float *D = debug_T12 + 12 * it;
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) D[r * 3 + c] = Rn[c * 3 + r];
        for (int r = 0; r < 3; ++r)
          D[9 + r] = -(D[r * 3 + 0] * tn[0] + D[r * 3 + 1] * tn[1] + D[r * 3 + 2] * tn[2]);
      }
      // mono: reference :112; stereo: :331 (count_left = n, exact in fp32 below 2^24)
      const float err_curr = STEREO ? tot[27] / (((float)n + tot[28]) * 0.5f)
                                    : tot[27] * (inv_n * 0.5f);
      const float delta_error = fabsf(err_curr - s_err_prev);
      const float dn = sqrtf(v0 * v0 + v1 * v1 + v2 * v2 + w0 * w0 + w1 * w1 + w2 * w2);
      ctl[1] = it + 1;
      if (lead) meta[0] = it + 1;
      if (dn < thr_step || delta_error < thr_cost) {
        if (lead) meta[1] = 1;
        ctl[0] = 1;  // converged: no Summary row (reference :116-121)
      } else {
        if (lead && it == max_it - 1) meta[1] = 0;
        if (lead && iters && n_rows < cap) {
          iters[n_rows].cost = err_curr;
          iters[n_rows].cost_change = delta_error;
          iters[n_rows].abs_step = dn;
        }
        ++n_rows;
        if (lead) meta[2] = n_rows;
        s_err_prev = err_curr;
      }
    }
    __syncthreads();
    if (ctl[0]) break;
  }
  // (with no iteration executed nothing was exchanged: T12 stays as given, and
  //  no workgroup may write it while another still reads it)
  if (tid == 0 && lead && ctl[1] > 0) {
    float nrm = 0.0f;
    for (int k = 0; k < 9; ++k) nrm += pose[k] * pose[k];
    if (isnan(nrm)) {
      meta[3] = BATCH ? 1 : 0;  // reference :159-167: do not update on NaN
    } else {
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T12[r * 3 + c] = pose[c * 3 + r];
      for (int r = 0; r < 3; ++r)
        T12[9 + r] = -(T12[r * 3 + 0] * pose[9] + T12[r * 3 + 1] * pose[10] +
                       T12[r * 3 + 2] * pose[11]);
    }
  }
}

// ---- planar 3-DoF (reference :401-615 mono, :617-900 stereo) -----------------
constexpr int kNred3 = 11;  // 6 upper H + 3 g + 1 err + 1 count of right-camera edges

// C = A * B and c = A * b + a for 3x3 row-major rotations (Eigen's Isometry
// product, linear part first)
__device__ __forceinline__ void po3_compose(const float *RA, const float *tA, const float *RB,
                                            const float *tB, float *RC, float *tC) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      RC[r * 3 + c] = RA[r * 3 + 0] * RB[0 * 3 + c] + RA[r * 3 + 1] * RB[1 * 3 + c] +
                      RA[r * 3 + 2] * RB[2 * 3 + c];
    tC[r] = (RA[r * 3 + 0] * tB[0] + RA[r * 3 + 1] * tB[1] + RA[r * 3 + 2] * tB[2]) + tA[r];
  }
}

// One camera's terms of one point (reference :1454-1583) added to acc.
// Lp = point in that camera, xb / yb = the INPUT point (the psi column uses it,
// :1491-1494), R6 = r11 r12 r21 r22 r31 r32 of that camera's camera-to-base
// rotation.
__device__ __forceinline__ void po3_edge(const float Lp[3], float xb, float yb, float cps,
                                         float sps, const float R6[6], float fx, float fy,
                                         float cx, float cy, float pu, float pv,
                                         float thr_huber, float thr_out, float acc[kNred3],
                                         uint8_t *mk) {
  const float iz = 1.0f / Lp[2];
  const float xiz = Lp[0] * iz, yiz = Lp[1] * iz;
  const float fxxiz = fx * xiz, fyyiz = fy * yiz;
  const float ru = (fxxiz + cx) - pu;
  const float rv = (fyyiz + cy) - pv;
  const float a1 = fx * iz, a2 = -fxxiz * iz, b1 = fy * iz, b2 = -fyyiz * iz;
  const float A = -sps * xb - cps * yb;
  const float B = cps * xb - sps * yb;
  float Ju[3], Jv[3];
  Ju[0] = a1 * R6[0] + a2 * R6[4];
  Ju[1] = a1 * R6[1] + a2 * R6[5];
  Ju[2] = Ju[0] * A + Ju[1] * B;
  Jv[0] = b1 * R6[2] + b2 * R6[4];
  Jv[1] = b1 * R6[3] + b2 * R6[5];
  Jv[2] = Jv[0] * A + Jv[1] * B;
  const float ars = fabsf(ru) + fabsf(rv);
  const bool hub = ars >= thr_huber;
  const float w = hub ? thr_huber / ars : 1.0f;
  const float wru = hub ? w * ru : ru, wrv = hub ? w * rv : rv;
  int k = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = r; c < 3; ++c) {
      const float hu = hub ? (w * Ju[r]) * Ju[c] : Ju[r] * Ju[c];
      const float hv = hub ? (w * Jv[r]) * Jv[c] : Jv[r] * Jv[c];
      acc[k++] += hu + hv;
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[6 + c] -= wru * Ju[c] + wrv * Jv[c];
  acc[9] += hub ? wru * ru : rv * rv;  // Q9, as in the 6-DoF path
  if (ars >= thr_out) *mk = 0;         // reference :524, :779, :813
}

// Thread 0: pose_b2b1(theta) and the camera poses it gives (reference
// :484-490, :718-727) into LDS.  pb = R (9) then t (3) of pose_b2b1,
// pl / pr = left / right camera_to_base1 (R then t), cs = cos, sin of psi.
__device__ __forceinline__ void po3_set_pose(const float *th, const Po3Params &P, bool stereo,
                                             float *pb, float *pl, float *pr, float *cs) {
  const float c = cosf(th[2]), s = sinf(th[2]);
  cs[0] = c;
  cs[1] = s;
  pb[0] = c; pb[1] = -s; pb[2] = 0.0f;
  pb[3] = s; pb[4] = c;  pb[5] = 0.0f;
  pb[6] = 0.0f; pb[7] = 0.0f; pb[8] = 1.0f;
  pb[9] = th[0]; pb[10] = th[1]; pb[11] = 0.0f;
  po3_compose(P.Rcb, P.tcb, pb, pb + 9, pl, pl + 9);
  if (stereo) po3_compose(P.Rrl, P.trl, pl, pl + 9, pr, pr + 9);
}

// The planar solver: the same one-launch shape as k_pose_only6 (co-resident
// workgroups, DPP + LDS sums, one grid barrier per iteration, every workgroup
// runs the same 3x3 solve and update), on theta = (x, y, psi) of pose_b2b1.
// The input points are base-1 coordinates; X_c = T_cb * T_b2b1(theta) * X.
// T12 (world_to_current) is only written, with pose_b2b1^-1 * base_to_camera
// (:549-551, :604-612), when at least one iteration ran and the pose is not NaN.
//
// BATCH (ba_pose_only_{mono,stereo}3_batch): B independent problems, one
// workgroup each, as k_pose_only6<STEREO, true>: gsync = offsets (B+1),
// partial = left intrinsics (B x 4), recs = the planar records (B x Po3Params,
// built on the host: the prior's psi is a host atan2), T12 (B x 12), iters
// (B x cap), debug_T12 (B x cap x 12), meta = ba_po_result records (status 0 =
// pose written, 1 = NaN, 2 = empty range and nothing else written); n, fx..cy
// and P1 are unused.  G = 1 at compile time: the arithmetic of a one-workgroup
// launch of k_pose_only3<STEREO, false>.  Single calls pass recs = nullptr.
template <bool STEREO, bool BATCH>
__global__ __launch_bounds__(kPoThreads) void k_pose_only3(
    const float *__restrict__ X3, const float *__restrict__ uv2,
    const float *__restrict__ uvr2, int n, float fx, float fy, float cx, float cy,
    const Po3Params P1, float *T12, uint8_t *mask, uint8_t *maskr, float thr_huber,
    float thr_step, float thr_cost, float thr_out, int max_it, PoIter *iters, int cap,
    int *meta, float *debug_T12, int *gsync, float *partial,
    const Po3Params *__restrict__ recs) {
  if constexpr (BATCH) {
    const unsigned b = blockIdx.x;
    const int o = gsync[b];
    n = gsync[b + 1] - o;
    meta += 4 * (size_t)b;
    if (n <= 0) {
      if (threadIdx.x == 0) {
        meta[0] = 0;
        meta[1] = 0;
        meta[2] = 0;
        meta[3] = 2;
      }
      return;
    }
    X3 += 3 * (size_t)o;
    uv2 += 2 * (size_t)o;
    mask += o;
    if (STEREO) {
      uvr2 += 2 * (size_t)o;
      maskr += o;
    }
    recs += b;
    fx = partial[4 * b];
    fy = partial[4 * b + 1];
    cx = partial[4 * b + 2];
    cy = partial[4 * b + 3];
    T12 += 12 * (size_t)b;
    if (iters) iters += (size_t)b * cap;
    if (debug_T12) debug_T12 += (size_t)b * cap * 12;
  }
  const Po3Params &P = BATCH ? *recs : P1;
  const int G = BATCH ? 1 : gridDim.x;
  const bool lead = BATCH ? true : blockIdx.x == 0;
  __shared__ float red[kPoWaves][kNred3];
  __shared__ float tots[kNred3];
  __shared__ float Hs[9], gs[3], tmps[3];
  __shared__ int trs[3];
  __shared__ float theta[3];   // parameter_b2b1_optimized
  __shared__ float pb[12];     // pose_b2b1_optimized: R (9) then t (3)
  __shared__ float pl[12], pr[12], cs[2];
  __shared__ float wpose[12];  // pose_world_to_current_optimized
  __shared__ int ctl[2];       // [0] = stop flag, [1] = iterations executed
  __shared__ float s_err_prev;
  __shared__ bool s_nan;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) {
    s_nan = false;
    for (int k = 0; k < 3; ++k) theta[k] = P.theta0[k];
    po3_set_pose(theta, P, STEREO, pb, pl, pr, cs);
    ctl[0] = 0;
    ctl[1] = 0;
    s_err_prev = 1e10f;
    if (lead) {
      meta[0] = 0;
      meta[1] = 1;
      meta[2] = 0;
      meta[3] = BATCH ? 0 : 1;
    }
  }
  int n_rows = 0;  // Summary rows logged so far (thread 0)
  __syncthreads();
  const float inv_n = 1.0f / (float)n;
  const float Rl6[6] = {P.Rcb[0], P.Rcb[1], P.Rcb[3], P.Rcb[4], P.Rcb[6], P.Rcb[7]};
  const float Rr6[6] = {P.Rrb[0], P.Rrb[1], P.Rrb[3], P.Rrb[4], P.Rrb[6], P.Rrb[7]};
  for (int it = 0; it < max_it; ++it) {
    float Rl[9], tl[3], Rr[9], tr[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rl[k] = pl[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tl[k] = pl[9 + k];
    if (STEREO) {
#pragma unroll
      for (int k = 0; k < 9; ++k) Rr[k] = pr[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) tr[k] = pr[9 + k];
    }
    const float cps = cs[0], sps = cs[1];
    float acc[kNred3];
#pragma unroll
    for (int k = 0; k < kNred3; ++k) acc[k] = 0.0f;
    // kU points per trip, loads issued together (as in k_pose_only6); two in
    // stereo, where four would spill
    constexpr int kU = STEREO ? 2 : 4;
    const int gstride = G * kPoThreads;
    for (int p0 = (BATCH ? 0u : blockIdx.x) * kPoThreads + tid; p0 < n; p0 += kU * gstride) {
      float Xb[kU][3], ub[kU][2], urb[kU][2];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int p = p0 + u * gstride;
        const int pc = p < n ? p : n - 1;
        Xb[u][0] = X3[3 * pc]; Xb[u][1] = X3[3 * pc + 1]; Xb[u][2] = X3[3 * pc + 2];
        ub[u][0] = uv2[2 * pc]; ub[u][1] = uv2[2 * pc + 1];
        if (STEREO) { urb[u][0] = uvr2[2 * pc]; urb[u][1] = uvr2[2 * pc + 1]; }
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int p = p0 + u * gstride;
        if (p >= n) break;
        float Lp[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
          Lp[r] = (Rl[r * 3 + 0] * Xb[u][0] + Rl[r * 3 + 1] * Xb[u][1] + Rl[r * 3 + 2] * Xb[u][2]) + tl[r];
        po3_edge(Lp, Xb[u][0], Xb[u][1], cps, sps, Rl6, fx, fy, cx, cy, ub[u][0], ub[u][1],
                 thr_huber, thr_out, acc, mask + p);
        if (STEREO) {
          const float pu = urb[u][0], pv = urb[u][1];
          if (!(pu < 0 || pv < 0)) {  // reference :785
            float Lr[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
              Lr[r] = (Rr[r * 3 + 0] * Xb[u][0] + Rr[r * 3 + 1] * Xb[u][1] + Rr[r * 3 + 2] * Xb[u][2]) + tr[r];
            po3_edge(Lr, Xb[u][0], Xb[u][1], cps, sps, Rr6, P.cam_r[0], P.cam_r[1], P.cam_r[2],
                     P.cam_r[3], pu, pv, thr_huber, thr_out, acc, maskr + p);
            acc[10] += 1.0f;
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kNred3; ++k) {
      const float s = wave_sum_f(acc[k]);
      if (lane == 0) red[wv][k] = s;
    }
    __syncthreads();
    if (tid < kNred3) {
      float sk = 0.0f;
#pragma unroll
      for (int w = 0; w < kPoWaves; ++w) sk += red[w][tid];
      tots[tid] = sk;
    }
    if (G > 1) {
      float *pbuf = partial + (size_t)(it & 1) * kPoMaxGroups * kNred3;
      if (tid < kNred3)
        __hip_atomic_store(&pbuf[blockIdx.x * kNred3 + tid], tots[tid], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      po_grid_barrier(gsync, (it + 1) * G);
      if (tid < kNred3) {
        float sk = 0.0f;
        for (int w = 0; w < G; ++w)
          sk += __hip_atomic_load(&pbuf[w * kNred3 + tid], __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
        tots[tid] = sk;
      }
    }
    __syncthreads();
    if (tid == 0) {
      float tot[kNred3];
#pragma unroll
      for (int k = 0; k < kNred3; ++k) tot[k] = tots[k];
      int k = 0;
      for (int r = 0; r < 3; ++r)
        for (int c = r; c < 3; ++c) {
          Hs[r * 3 + c] = tot[k];
          Hs[c * 3 + r] = tot[k];
          ++k;
        }
      for (int r = 0; r < 3; ++r) Hs[r * 3 + r] *= (1.0f + 1e-5f);  // :532
      for (int c = 0; c < 3; ++c) gs[c] = tot[6 + c];
      ldlt_solve<3>(Hs, gs, trs, tmps);  // delta_param, :534
      const float dx = gs[0], dy = gs[1], dpsi = gs[2];
      // delta_pose * pose_b2b1_optimized, x / y re-read, psi += delta (:536-547)
      const float cd = cosf(dpsi), sd = sinf(dpsi);
      const float Rd[9] = {cd, -sd, 0.0f, sd, cd, 0.0f, 0.0f, 0.0f, 1.0f};
      const float td[3] = {dx, dy, 0.0f};
      float Rn[9], tn[3];
      po3_compose(Rd, td, pb, pb + 9, Rn, tn);
      float nrm = 0.0f;
      for (int q = 0; q < 9; ++q) {
        pb[q] = Rn[q];
        nrm += Rn[q] * Rn[q];
      }
      for (int q = 0; q < 3; ++q) pb[9 + q] = tn[q];
      s_nan = isnan(nrm);  // the write-back test, on this product (:604)
      theta[0] = tn[0];
      theta[1] = tn[1];
      theta[2] += dpsi;
      // pose_b2b1_optimized^-1 * base_to_camera (:549-551)
      float Ri[9], ti[3];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Ri[r * 3 + c] = Rn[c * 3 + r];
      for (int r = 0; r < 3; ++r)
        ti[r] = -(Ri[r * 3 + 0] * tn[0] + Ri[r * 3 + 1] * tn[1] + Ri[r * 3 + 2] * tn[2]);
      po3_compose(Ri, ti, P.Rbc, P.tbc, wpose, wpose + 9);
      if (lead && debug_T12 && it < cap)
        for (int q = 0; q < 12; ++q) debug_T12[12 * it + q] = wpose[q];
      // mono :553; stereo :842 (count_left = n, exact in fp32 below 2^24)
      const float err_curr = STEREO ? tot[9] / (((float)n + tot[10]) * 0.5f)
                                    : tot[9] * (inv_n * 0.5f);
      const float delta_error = fabsf(err_curr - s_err_prev);
      const float dn = sqrtf(dx * dx + dy * dy + dpsi * dpsi);
      ctl[1] = it + 1;
      if (lead) meta[0] = it + 1;
      if (dn < thr_step || delta_error < thr_cost) {
        if (lead) meta[1] = 1;
        ctl[0] = 1;  // converged: no Summary row (:556-564, :845-850)
      } else {
        if (lead && it == max_it - 1) meta[1] = 0;
        if (lead && iters && n_rows < cap) {
          iters[n_rows].cost = err_curr;
          iters[n_rows].cost_change = delta_error;
          iters[n_rows].abs_step = dn;
        }
        ++n_rows;
        if (lead) meta[2] = n_rows;
        s_err_prev = err_curr;
        po3_set_pose(theta, P, STEREO, pb, pl, pr, cs);  // next iteration's linearisation point
      }
    }
    __syncthreads();
    if (ctl[0]) break;
  }
  if (tid == 0 && lead && ctl[1] > 0) {
    if (s_nan) {
      meta[3] = BATCH ? 1 : 0;  // :604-612: do not update on NaN
    } else {
      for (int q = 0; q < 12; ++q) T12[q] = wpose[q];
    }
  }
}

}  // namespace

// workgroups for n points: about kPoPointsPerThread points per thread
static int po_groups(int n) {
  int g = (n + kPoThreads * kPoPointsPerThread - 1) / (kPoThreads * kPoPointsPerThread);
  return g < 1 ? 1 : (g > kPoMaxGroups ? kPoMaxGroups : g);
}
int pose_only_sync_ints() { return 2; }
int pose_only_partial_floats() { return 2 * kPoMaxGroups * kNred; }

int pose_only_mono6_device(const float *dX3, const float *duv2, int n, float fx,
                           float fy, float cx, float cy, float *dT12,
                           uint8_t *dmask, float thr_huber, float thr_step,
                           float thr_cost, float thr_out, int max_it,
                           PoIter *d_iters, int cap, int *d_meta,
                           float *d_debug, int *d_gsync, float *d_partial, hipStream_t s) {
  // d_gsync must be zero on entry (the caller's single H2D copy covers it)
  hipLaunchKernelGGL((k_pose_only6<false, false>), dim3(po_groups(n)), dim3(kPoThreads), 0, s, dX3, duv2,
                     (const float *)nullptr, n, fx, fy, cx, cy, (const float *)nullptr, dT12,
                     dmask, (uint8_t *)nullptr, thr_huber, thr_step, thr_cost, thr_out, max_it,
                     d_iters, cap, d_meta, d_debug, d_gsync, d_partial);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pose_only_stereo6_device(const float *dX3, const float *duvl2, const float *duvr2, int n,
                             float fx, float fy, float cx, float cy, const float *d_cam_r16,
                             float *dT12, uint8_t *dmask_l, uint8_t *dmask_r, float thr_huber,
                             float thr_step, float thr_cost, float thr_out, int max_it,
                             PoIter *d_iters, int cap, int *d_meta, float *d_debug,
                             int *d_gsync, float *d_partial, hipStream_t s) {
  // d_gsync must be zero on entry (the caller's single H2D copy covers it)
  hipLaunchKernelGGL((k_pose_only6<true, false>), dim3(po_groups(n)), dim3(kPoThreads), 0, s, dX3, duvl2,
                     duvr2, n, fx, fy, cx, cy, d_cam_r16, dT12, dmask_l, dmask_r, thr_huber,
                     thr_step, thr_cost, thr_out, max_it, d_iters, cap, d_meta, d_debug, d_gsync,
                     d_partial);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pose_only6_batch_device(bool stereo, int B, const int *d_offsets, const float *dX3,
                            const float *duvl2, const float *duvr2, const float *d_intr_l4,
                            const float *d_camr16, float *dT12, uint8_t *dmask_l, uint8_t *dmask_r,
                            float thr_huber, float thr_step, float thr_cost, float thr_out,
                            int max_it, PoIter *d_iters, int cap, int *d_res, float *d_debug,
                            hipStream_t s) {
  // per-batch arrays in the slots k_pose_only6<STEREO, true> re-points (see there)
  int *offs = const_cast<int *>(d_offsets);
  float *intr = const_cast<float *>(d_intr_l4);
  if (stereo)
    hipLaunchKernelGGL((k_pose_only6<true, true>), dim3(B), dim3(kPoThreads), 0, s, dX3, duvl2,
                       duvr2, 0, 0.0f, 0.0f, 0.0f, 0.0f, d_camr16, dT12, dmask_l, dmask_r,
                       thr_huber, thr_step, thr_cost, thr_out, max_it, d_iters, cap, d_res, d_debug,
                       offs, intr);
  else
    hipLaunchKernelGGL((k_pose_only6<false, true>), dim3(B), dim3(kPoThreads), 0, s, dX3, duvl2,
                       (const float *)nullptr, 0, 0.0f, 0.0f, 0.0f, 0.0f, (const float *)nullptr,
                       dT12, dmask_l, (uint8_t *)nullptr, thr_huber, thr_step, thr_cost, thr_out,
                       max_it, d_iters, cap, d_res, d_debug, offs, intr);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pose_only_planar3_device(bool stereo, const float *dX3, const float *duvl2,
                             const float *duvr2, int n, float fx, float fy, float cx, float cy,
                             const Po3Params &P, float *dT12, uint8_t *dmask_l, uint8_t *dmask_r,
                             float thr_huber, float thr_step, float thr_cost, float thr_out,
                             int max_it, PoIter *d_iters, int cap, int *d_meta, float *d_debug,
                             int *d_gsync, float *d_partial, hipStream_t s) {
  // d_gsync must be zero on entry (the caller's single H2D copy covers it)
  static_assert(kNred3 <= kNred, "partial-sum buffer sized for the 6-DoF sums");
  if (stereo)
    hipLaunchKernelGGL((k_pose_only3<true, false>), dim3(po_groups(n)), dim3(kPoThreads), 0, s, dX3,
                       duvl2, duvr2, n, fx, fy, cx, cy, P, dT12, dmask_l, dmask_r, thr_huber, thr_step,
                       thr_cost, thr_out, max_it, d_iters, cap, d_meta, d_debug, d_gsync, d_partial,
                       (const Po3Params *)nullptr);
  else
    hipLaunchKernelGGL((k_pose_only3<false, false>), dim3(po_groups(n)), dim3(kPoThreads), 0, s, dX3,
                       duvl2, (const float *)nullptr, n, fx, fy, cx, cy, P, dT12, dmask_l,
                       (uint8_t *)nullptr, thr_huber, thr_step, thr_cost, thr_out, max_it, d_iters,
                       cap, d_meta, d_debug, d_gsync, d_partial, (const Po3Params *)nullptr);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int pose_only3_batch_device(bool stereo, int B, const int *d_offsets, const float *dX3,
                            const float *duvl2, const float *duvr2, const float *d_intr_l4,
                            const float *d_rec52, float *dT12, uint8_t *dmask_l, uint8_t *dmask_r,
                            float thr_huber, float thr_step, float thr_cost, float thr_out,
                            int max_it, PoIter *d_iters, int cap, int *d_res, float *d_debug,
                            hipStream_t s) {
  // per-batch arrays in the slots k_pose_only3<STEREO, true> re-points (see there)
  int *offs = const_cast<int *>(d_offsets);
  float *intr = const_cast<float *>(d_intr_l4);
  const Po3Params *recs = reinterpret_cast<const Po3Params *>(d_rec52);
  const Po3Params unused{};
  if (stereo)
    hipLaunchKernelGGL((k_pose_only3<true, true>), dim3(B), dim3(kPoThreads), 0, s, dX3, duvl2,
                       duvr2, 0, 0.0f, 0.0f, 0.0f, 0.0f, unused, dT12, dmask_l, dmask_r, thr_huber,
                       thr_step, thr_cost, thr_out, max_it, d_iters, cap, d_res, d_debug, offs, intr,
                       recs);
  else
    hipLaunchKernelGGL((k_pose_only3<false, true>), dim3(B), dim3(kPoThreads), 0, s, dX3, duvl2,
                       (const float *)nullptr, 0, 0.0f, 0.0f, 0.0f, 0.0f, unused, dT12, dmask_l,
                       (uint8_t *)nullptr, thr_huber, thr_step, thr_cost, thr_out, max_it, d_iters,
                       cap, d_res, d_debug, offs, intr, recs);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace ba
