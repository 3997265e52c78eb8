// ba_chol_lds.h — Cholesky factorisation and solve of a small SPD system held in LDS by
// ONE 256-thread workgroup: the tail block of the level-scheduled reduced solve
// (k_chol_tail, ba_dense.hip) and the whole reduced camera system of a batched window
// problem (ba_batch.hip), and the inverse of that system from its factor.  Internal.
#ifndef BA_CHOL_LDS_H_
#define BA_CHOL_LDS_H_

#include "ba_device.h"
#include "ba_tile16.h"

namespace ba {

// (kTailCols: ba_dense_sched.h)
constexpr int kTailLS = kTailCols + 16 + 1;  // column stride of the LDS image (rows + rhs block + pad)
constexpr int kTailES = 17;

// dropped pivots are counted per handle (ba_get_dropped_pivots) or per problem of a batch;
// the integer atomic runs only when a factorisation actually meets one
__device__ __forceinline__ void count_bad_pivots(int *bad, int n, int lane) {
  if (bad && n > 0 && lane == 0) atomicAdd(bad, n);
}

// Lb[c*LS + r]: column-major lower image of nbt = 16*NPt columns (unit diagonal on padding
// columns), rows nbt .. nbt+15 the rhs block (row nbt = rhs); Eb[p] receives E_pp = L_pp^-T
// (zeroed by the caller); xs receives x.  Left-looking 16-column panels (MFMA panel update
// and TRSM, wave 0 factors the 16x16 diagonal tiles), the rhs forward-substituted as one
// more row tile, block back substitution by wave 0.  Unpivoted: a pivot <= 1e-300 zeroes
// its column and solution component and is counted in *bad.  Starts after a barrier of the
// caller; the caller synchronises before it reads xs.
template <int NPt, bool PAIR, int LS>
__device__ __forceinline__ void chol_lds_factor_solve(double *Lb, double (*Eb)[16 * kTailES], double *xs,
                                                      int *bad) {
  typedef double v4f64 __attribute__((ext_vector_type(4)));
  constexpr int nbt = 16 * NPt, ES = kTailES;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;

  // Macro-steps.  PAIR: the first level of the block has TWO 32-column tiles
  // (panels 0,1 and 2,3).  Tiles of one level are independent (the tile between
  // them is structurally zero), so their panels are processed side by side:
  // {0,2}, {1,3}, then 4, 5 — four sequential 16x16 factorisations instead of six.
  constexpr int NG = PAIR ? NPt - 2 : NPt;
#pragma unroll
  for (int m = 0; m < NG; ++m) {
    const int p0 = PAIR ? (m < 2 ? m : m + 2) : m;
    const bool two = PAIR && m < 2;
    // this wave's panel: waves 0,1 -> p0 and waves 2,3 -> p0 + 2 in a paired step
    const int p = (two && wv >= 2) ? p0 + 2 : p0;
    const int w2 = two ? (wv & 1) : wv, nw = two ? 2 : 4;
    // columns that can contribute to panel p: from its own tile on in a paired
    // step (the other tile's columns are zero in these rows), else all earlier ones
    const int kc0 = two ? 32 * (p >> 1) : 0;
    // (1) left-looking update: tile (ti,p) -= sum_kt L(ti,kt) L(p,kt)^T, ti = p .. NPt
    if (m > 0) {
      for (int ti = p + w2; ti <= NPt; ti += nw) {
        v4f64 acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr];
        for (int kc = kc0; kc < 16 * p; kc += 4) {
          const double a = -Lb[(kc + lk) * LS + 16 * p + lr];
          const double b = Lb[(kc + lk) * LS + 16 * ti + lr];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr] = acc[g];
      }
      __syncthreads();
    }
    // (2) factor the diagonal tile(s): wave 0 (and wave 2 for the second panel of a paired step)
    if (wv == 0 || (two && wv == 2)) {
      const int r = lr, q = lk;
      double g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * j + q;
        g[j] = (r >= c) ? Lb[(16 * p + c) * LS + 16 * p + r] : 0.0;
      }
      double dinv;
      count_bad_pivots(bad, tile16::tile16_potrf_inv2(g, lane, dinv), lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * j + q;
        if (r >= c) Lb[(16 * p + c) * LS + 16 * p + r] = g[j];
        if (r < c) Eb[p][r * ES + c] = g[j];
        if (r == c) Eb[p][r * ES + c] = dinv;
      }
    }
    __syncthreads();
    // (3) TRSM of the tiles below (incl. the rhs block): X = T * E_pp
    for (int ti = p + 1 + w2; ti <= NPt; ti += nw) {
      v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const double a = Eb[p][(lk + 4 * g) * ES + lr];
        const double b = Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
      // all reads of this tile precede the writes within the wave
#pragma unroll
      for (int g = 0; g < 4; ++g) Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr] = acc[g];
    }
    __syncthreads();
  }
  // (4) L^T x = y by block back substitution (wave 0): y is row 0 of the rhs block,
  //     x_p = E_pp (y_p - sum_{u>p} L_up^T x_u)
  if (wv == 0) {
    const int i = lr, q = lk;
#pragma unroll
    for (int p = NPt - 1; p >= 0; --p) {
      double acc = 0.0;
#pragma unroll
      for (int u = p + 1; u < NPt; ++u)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int row = 16 * u + 4 * q + rr;
          acc += Lb[(16 * p + i) * LS + row] * xs[row];
        }
      acc += __shfl_xor(acc, 16, 64);
      acc += __shfl_xor(acc, 32, 64);
      const double wvv = Lb[(16 * p + i) * LS + nbt] - acc;
      double px = 0.0;
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const int c2 = 4 * q + cc;
        px += Eb[p][i * ES + c2] * __shfl(wvv, c2, 64);
      }
      px += __shfl_xor(px, 16, 64);
      px += __shfl_xor(px, 32, 64);
      if (q == 0) xs[16 * p + i] = px;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

// S^-1 = L^-T L^-1 of the system chol_lds_factor_solve left in the image, in place.  On
// entry the lower triangle of Lb holds L and Eb[p] = L_pp^-T; the off-diagonal tiles of the
// upper triangle are free.
//   (1) Z = L^-1 by block triangular inversion, Z_pp = E_pp^T and
//         Z_tp = -E_tt^T sum_{p <= u < t} L_tu Z_up            (t > p),
//       stored as tile (p, t) of the upper triangle: Z_tp(a, b) at Lb[(16 t + a) LS + 16 p + b].
//       Tiles of one distance t - p depend on smaller distances only: one level per distance,
//       its tiles dealt to the four waves.
//   (2) [S^-1]_pq = sum_{u >= p} Z_up^T Z_uq (p >= q) into the lower triangle, the diagonal
//       tiles in full.  L is gone afterwards; Eb is kept.
// Every sum is an MFMA chain in ascending tile order, so a padding tile (unit diagonal,
// Z = identity there) adds exact zeros after the last real term: the same bits at any NPt.
// Starts after a barrier of the caller and ends with one.
template <int NPt, int LS>
__device__ __forceinline__ void chol_lds_inverse(double *Lb, double (*Eb)[16 * kTailES]) {
  typedef double v4f64 __attribute__((ext_vector_type(4)));
  constexpr int ES = kTailES;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  // operand maps: A[i = lr][k = lk + 4 s], B[k = lk + 4 s][j = lr], D register g = D[lk + 4 g][lr]
#pragma unroll
  for (int dist = 1; dist < NPt; ++dist) {
    for (int p = wv; p + dist < NPt; p += 4) {
      const int t = p + dist;
      v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};  // R(a, b) = sum_u L_tu Z_up, i = a, j = b
      for (int u = p; u < t; ++u)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int k = lk + 4 * s;
          const double a = Lb[(16 * u + k) * LS + 16 * t + lr];
          const double b = (u == p) ? Eb[p][lr * ES + k] : Lb[(16 * u + k) * LS + 16 * p + lr];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
      v4f64 z = (v4f64){0.0, 0.0, 0.0, 0.0};  // Z_tp = -E_tt^T R: an accumulator is the next B operand
#pragma unroll
      for (int s = 0; s < 4; ++s)
        z = __builtin_amdgcn_mfma_f64_16x16x4f64(-Eb[t][(lk + 4 * s) * ES + lr], acc[s], z, 0, 0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) Lb[(16 * t + lk + 4 * g) * LS + 16 * p + lr] = z[g];
    }
    __syncthreads();
  }
  // (2) D[b][a] = sum_u sum_k Z_uq(k, b) Z_up(k, a) -> Lb[(16 q + b) LS + 16 p + a]
  for (int task = wv; task < NPt * (NPt + 1) / 2; task += 4) {
    int p = 0;
    while ((p + 1) * (p + 2) / 2 <= task) ++p;
    const int q = task - p * (p + 1) / 2;
    v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
    for (int u = p; u < NPt; ++u)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int k = lk + 4 * s;
        const double a = (u == q) ? Eb[q][lr * ES + k] : Lb[(16 * u + k) * LS + 16 * q + lr];
        const double b = (u == p) ? Eb[p][lr * ES + k] : Lb[(16 * u + k) * LS + 16 * p + lr];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
#pragma unroll
    for (int g = 0; g < 4; ++g) Lb[(16 * q + lk + 4 * g) * LS + 16 * p + lr] = acc[g];
  }
  __syncthreads();
}

// Partial factorisation of the image of chol_lds_factor_solve: eliminate the first T
// 16-column panels (T <= NPt, uniform over the workgroup) and leave the Schur complement of
// the rest in place.
//   panels p < T    steps (1)-(3) of chol_lds_factor_solve, the rhs row tile included;
//   panels p >= T   only the left-looking update (1) over the eliminated columns kc < 16 T,
//                   tiles p .. NPt.  These panels read columns below 16 T only and write
//                   their own, so they need no barrier between them: their tiles are dealt
//                   to the four waves as one list.
// Afterwards the lower triangle from column 16 T on holds S_kk - S_km S_mm^-1 S_mk (the
// diagonal tiles are full 16x16 MFMA results of a lower-only image: read row >= column
// only), and row nbt of those columns r_k - S_km S_mm^-1 r_m.  Every tile is one MFMA chain
// over kc ascending from 0, whose length depends on T and not on NPt, and trailing padding
// tiles add nothing to another tile: the same bits at any NPt.  Pivots as in
// chol_lds_factor_solve, counted for the eliminated panels only.  Eb (zeroed by the caller)
// receives E_pp for p < T.  Starts after a barrier of the caller and ends with one.
template <int NPt, int LS>
__device__ __forceinline__ void chol_lds_partial(double *Lb, double (*Eb)[16 * kTailES], const int T, int *bad) {
  typedef double v4f64 __attribute__((ext_vector_type(4)));
  constexpr int ES = kTailES;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  for (int p = 0; p < T; ++p) {
    if (p > 0) {
      for (int ti = p + wv; ti <= NPt; ti += 4) {
        v4f64 acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr];
        for (int kc = 0; kc < 16 * p; kc += 4) {
          const double a = -Lb[(kc + lk) * LS + 16 * p + lr];
          const double b = Lb[(kc + lk) * LS + 16 * ti + lr];
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr] = acc[g];
      }
      __syncthreads();
    }
    if (wv == 0) {
      const int r = lr, q = lk;
      double g[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * j + q;
        g[j] = (r >= c) ? Lb[(16 * p + c) * LS + 16 * p + r] : 0.0;
      }
      double dinv;
      count_bad_pivots(bad, tile16::tile16_potrf_inv2(g, lane, dinv), lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * j + q;
        if (r >= c) Lb[(16 * p + c) * LS + 16 * p + r] = g[j];
        if (r < c) Eb[p][r * ES + c] = g[j];
        if (r == c) Eb[p][r * ES + c] = dinv;
      }
    }
    __syncthreads();
    for (int ti = p + 1 + wv; ti <= NPt; ti += 4) {
      v4f64 acc = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const double a = Eb[p][(lk + 4 * g) * ES + lr];
        const double b = Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
      // all reads of this tile precede the writes within the wave
#pragma unroll
      for (int g = 0; g < 4; ++g) Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr] = acc[g];
    }
    __syncthreads();
  }
  if (T > 0) {
    // trailing update: tile (ti, p), T <= p <= ti <= NPt with p < NPt, row-major task list
    const int R = NPt - T, n_task = R * (R + 1) / 2 + R;
    for (int task = wv; task < n_task; task += 4) {
      int pr = 0, rem = task;
      while (rem >= R + 1 - pr) {
        rem -= R + 1 - pr;
        ++pr;
      }
      const int p = T + pr, ti = p + rem;
      v4f64 acc;
#pragma unroll
      for (int g = 0; g < 4; ++g) acc[g] = Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr];
      for (int kc = 0; kc < 16 * T; kc += 4) {
        const double a = -Lb[(kc + lk) * LS + 16 * p + lr];
        const double b = Lb[(kc + lk) * LS + 16 * ti + lr];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) Lb[(16 * p + lk + 4 * g) * LS + 16 * ti + lr] = acc[g];
    }
  }
  __syncthreads();
}

}  // namespace ba
#endif  // BA_CHOL_LDS_H_
