// ba_cov_sweep.h — the forward sweep of the covariance kernels, once: k_cov_solve<NB>
// (ba_cov.hip, the handle path) and k_graph_cov_solve<G, NB> (ba_graph_kernels.hip, the pose graphs)
// call it and differ only in what they do with the Gram matrix.  Device only, forced inline.
#ifndef BA_COV_SWEEP_H_
#define BA_COV_SWEEP_H_

#include <hip/hip_runtime.h>

namespace ba {

typedef double cov_v4f64 __attribute__((ext_vector_type(4)));

// MFMA operand maps (v_mfma_f64_16x16x4_f64): lane (lr = lane & 15, lk = lane >> 4) gives
// A[i = lr][k = lk] and B[k = lk][j = lr]; accumulator register g is D[i = lk + 4 g][j = lr].
// Here i = row of the tile, j = right-hand side: an accumulator register is 16 consecutive
// columns of one workspace row (128 contiguous bytes), and — k-step g taken over the rows
// k = lk + 4 g — the result of one product is the B operand of the next as it stands.
//
// One wave, its 16 right-hand sides in the columns Zc[0 .. 15] of the workspace (Zc: this
// lane's column lr, bw doubles per row): X = L^-1 E over the row tiles t0 .. ncb - 1, X left
// in the workspace, and the Gram matrix X^T X returned in the accumulator layout.
template <int NB>
__device__ __forceinline__ cov_v4f64 cov_sweep(const double *__restrict__ L, const int ld,
                                               const double *__restrict__ Ldiag, const int ncb,
                                               const int *__restrict__ trow_ptr,
                                               const int *__restrict__ trow, const int t0, double *Zc,
                                               const int bw) {
  typedef cov_v4f64 v4f64;
  constexpr int NP = NB / 16;
  constexpr int WS = NB * NB + NP * 256;
  const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4;
  v4f64 G = (v4f64){0.0, 0.0, 0.0, 0.0};
  for (int t = t0; t < ncb; ++t) {
    v4f64 acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[p][q] = Zc[(size_t)(t * NB + 16 * p + lk + 4 * q) * bw];
    const int e = trow_ptr[t + 1];
    for (int a = trow_ptr[t]; a < e; ++a) {
      const int s = trow[a];
      if (s < t0) continue;  // (wave-uniform) X_s = 0
      const double *Lc = L + (size_t)s * NB * ld + t * NB + lr;  // column s NB + k, row t NB + r
      const double *Zs = Zc + (size_t)s * NB * bw;
#pragma unroll 4
      for (int kk = 0; kk < NB / 4; ++kk) {
        const int k = 4 * kk + lk;
        const double bz = Zs[(size_t)k * bw];
#pragma unroll
        for (int p = 0; p < NP; ++p)
          acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(-Lc[(size_t)k * ld + 16 * p], bz, acc[p], 0, 0, 0);
      }
    }
    // X_p = L_pp^-1 (R_p - sum_{q < p} L_pq X_q): factor tile column-major, zero above the
    // diagonal; Et[p][k][c] = (L_pp^-T)[k][c], so L_pp^-1[i][k] = Et[p][k][i]
    const double *Ld = Ldiag + (size_t)t * WS;
    const double *Et = Ld + NB * NB;
    v4f64 X[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      v4f64 r = acc[p];
#pragma unroll
      for (int q = 0; q < p; ++q)
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4)
          r = __builtin_amdgcn_mfma_f64_16x16x4f64(-Ld[(16 * q + lk + 4 * k4) * NB + 16 * p + lr], X[q][k4], r, 0, 0, 0);
      v4f64 o = (v4f64){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4)
        o = __builtin_amdgcn_mfma_f64_16x16x4f64(Et[p * 256 + (lk + 4 * k4) * 16 + lr], r[k4], o, 0, 0, 0);
      X[p] = o;
#pragma unroll
      for (int q = 0; q < 4; ++q) Zc[(size_t)(t * NB + 16 * p + lk + 4 * q) * bw] = o[q];
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) G = __builtin_amdgcn_mfma_f64_16x16x4f64(o[k4], o[k4], G, 0, 0, 0);
    }
    __syncthreads();  // the rows just stored are read back by other lanes of this wave
  }
  return G;
}

}  // namespace ba
#endif  // BA_COV_SWEEP_H_
