// ba_pgraph_cov.hip — covariance blocks of a pose graph and the chi-square gate for loop-closure
// candidates (ba_pgraph_covariance / ba_pgraph_gate, include/ba_hip.h).
//
// With H = L L^T the tile Cholesky that dense_factor_solve leaves in the graph's dense image at
// lambda = 0, Sigma = H^-1 and Z_j = L^-1 E_j (the six identity columns of pose j):
//   Sigma_jj = Z_j^T Z_j,   Sigma_jk = Z_j^T Z_k.
// One wave owns 16 right-hand sides: the columns of one pose in 0..5, of a second in 6..11.  It
// sweeps them with cov_sweep<NB> (ba_cov_sweep.h: the sweep of ba_covariance's k_cov_solve), and
// its 16x16 Gram matrix holds Sigma_jj, Sigma_kk and Sigma_jk at once.  What the wave does with
// them is the epilogue, through LDS:
//   kind 0 (two selected poses)  the two diagonal blocks
//   kind 1 (a pair j, k)         Sigma_jk (if asked for) and, with E = T_j T_k^-1 at the current
//                                poses and Ad = Ad(E) (rel_E / rel_Ad of ba_rel_fn.h),
//                                Sigma_E = Sigma_jj - Sigma_jk Ad^T - Ad Sigma_kj + Ad Sigma_kk Ad^T
//   kind 2 (a candidate)         also r = se3_log(E Z^-1) (rel_log), P = Sigma_E + Omega_z^-1 and
//                                d2 = r^T P^-1 r: two 6x6 Cholesky solves in plain fp64; a pivot of
//                                P that is not positive gives d2 = NaN
// A fixed member of a pair has no column: its blocks of the Gram matrix are exactly zero and the
// formula above is the reduced one.  No atomics, one writer per element, every sum in a fixed
// order: a block has the same bits run to run, in any selection and any batch split.
#include "ba_cov_sweep.h"
#include "ba_device.h"
#include "ba_device_fn.h"
#include "ba_pgraph_host.h"
#include "ba_rel_fn.h"

namespace ba {

namespace {

// identity columns of the group's optimisable members into the (zeroed) workspace
__global__ __launch_bounds__(64) void k_pgcov_rhs(const PgCovGroup *__restrict__ groups, double *Zw, int bw,
                                                  const int *__restrict__ pose_col) {
  const int lane = threadIdx.x;
  if (lane >= 12) return;
  const int a = lane / 6, r = lane - 6 * a;
  const int j = groups[blockIdx.x].opt[a];
  if (j >= 0) Zw[(size_t)(pose_col[j] + r) * bw + kCovGroupCols * blockIdx.x + 6 * a + r] = 1.0;
}

// In-place Cholesky of the 6x6 matrix A (row-major, LDS; the lower triangle is read and
// replaced by the factor); false at a pivot that is not positive.  One lane.
__device__ __forceinline__ bool chol6(double *A) {
  for (int c = 0; c < 6; ++c) {
    double d = A[c * 6 + c];
    for (int m = 0; m < c; ++m) d -= A[c * 6 + m] * A[c * 6 + m];
    if (!(d > 0.0)) return false;
    const double s = sqrt(d);
    A[c * 6 + c] = s;
    for (int r = c + 1; r < 6; ++r) {
      double v = A[r * 6 + c];
      for (int m = 0; m < c; ++m) v -= A[r * 6 + m] * A[c * 6 + m];
      A[r * 6 + c] = v / s;
    }
  }
  return true;
}
// x <- (L L^T)^-1 x for the factor chol6 left in A (x: 6 doubles in LDS, stride xs).  One lane.
__device__ __forceinline__ void chol6_solve(const double *A, double *x, const int xs) {
  for (int r = 0; r < 6; ++r) {
    double v = x[r * xs];
    for (int m = 0; m < r; ++m) v -= A[r * 6 + m] * x[m * xs];
    x[r * xs] = v / A[r * 6 + r];
  }
  for (int r = 5; r >= 0; --r) {
    double v = x[r * xs];
    for (int m = r + 1; m < 6; ++m) v -= A[m * 6 + r] * x[m * xs];
    x[r * xs] = v / A[r * 6 + r];
  }
}

template <int NB>
__global__ __launch_bounds__(64) void k_pgcov_solve(const double *__restrict__ L, int ld,
                                                    const double *__restrict__ Ldiag, int ncb,
                                                    const int *__restrict__ trow_ptr,
                                                    const int *__restrict__ trow,
                                                    const PgCovGroup *__restrict__ groups, double *Zw, int bw,
                                                    const double *__restrict__ poses,
                                                    const double *__restrict__ cand_val, PgCovOut out) {
  __shared__ double sG[256];                       // the Gram matrix, row-major
  __shared__ double sAd[36], sA[36], sS[36], sW[36], sP[36], sr[6], sy[6];
  const PgCovGroup g = groups[blockIdx.x];
  const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4;
  double *Zc = Zw + kCovGroupCols * blockIdx.x + lr;  // this lane's column
  const cov_v4f64 G = cov_sweep<NB>(L, ld, Ldiag, ncb, trow_ptr, trow, g.t0, Zc, bw);
#pragma unroll
  for (int q = 0; q < 4; ++q) sG[(lk + 4 * q) * 16 + lr] = G[q];
  __syncthreads();
  if (g.kind == kPgCovPoses) {  // the diagonal blocks
    for (int e = lane; e < 72; e += 64) {
      const int a = e / 36, q = e - 36 * a, r = q / 6, c = q - 6 * r;
      if (g.slot[a] >= 0) out.pose36[(size_t)g.slot[a] * 36 + q] = sG[(6 * a + r) * 16 + 6 * a + c];
    }
    return;
  }
  const size_t slot = (size_t)g.slot[0];
  // a candidate's Z (12) and Omega_z (36, mirrored by the host)
  const double *val = g.kind == kPgCovCand ? cand_val + slot * 48 : nullptr;
  if (lane == 0) {
    double RE[9], tE[3];
    rel_E(make_int4(g.pose[0], g.pose[1], 0, 0), poses, RE, tE);
    rel_Ad(RE, tE, sAd);
    if (g.kind == kPgCovCand) {
      double rr[6];
      rel_log(RE, tE, val, rr);
#pragma unroll
      for (int a = 0; a < 6; ++a) sr[a] = sy[a] = rr[a];
    }
  }
  __syncthreads();
  const int r0 = lane / 6, c0 = lane - 6 * r0;  // lanes 0..35: one element of a 6x6 block each
  if (lane < 36) {  // A = Ad Sigma_kk
    double acc = 0.0;
    for (int m = 0; m < 6; ++m) acc += sAd[r0 * 6 + m] * sG[(6 + m) * 16 + 6 + c0];
    sA[lane] = acc;
  }
  __syncthreads();
  if (lane < 36) {
    // element (r0, c0) of Sigma_E from the expression of its lower-triangle twin, so that the
    // block is symmetric to the bit (Sigma_kj[m][c] = Sigma_jk[c][m], the Gram matrix is)
    const int a = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
    double t1 = 0.0, t2 = 0.0, t3 = 0.0;
    for (int m = 0; m < 6; ++m) {
      t1 += sG[a * 16 + 6 + m] * sAd[c * 6 + m];
      t2 += sAd[a * 6 + m] * sG[c * 16 + 6 + m];
      t3 += sA[a * 6 + m] * sAd[c * 6 + m];
    }
    const double v = ((sG[a * 16 + c] - t1) - t2) + t3;
    sS[lane] = v;
    out.rel36[slot * 36 + lane] = v;
    if (out.cross36) out.cross36[slot * 36 + lane] = sG[r0 * 16 + 6 + c0];
    if (g.kind == kPgCovCand) sW[lane] = val[12 + lane];
  }
  if (g.kind != kPgCovCand) return;
  __syncthreads();
  // Omega_z^-1: the factor once, then one solve per identity column (lanes 0..5), in sP
  __shared__ int ok;
  if (lane == 0) ok = chol6(sW) ? 1 : 0;
  if (lane < 36) sP[lane] = r0 == c0 ? 1.0 : 0.0;
  __syncthreads();
  if (lane < 6 && ok) chol6_solve(sW, sP + lane, 6);
  __syncthreads();
  double pv = 0.0;
  if (lane < 36) {  // P = Sigma_E + Omega_z^-1, the inverse read from its lower-triangle twin
    const int a = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
    pv = sS[lane] + sP[a * 6 + c];
  }
  __syncthreads();
  if (lane < 36) {
    sW[lane] = pv;
    if (out.innov36) out.innov36[slot * 36 + lane] = ok ? pv : __builtin_nan("");
  }
  if (lane < 6 && out.r6) out.r6[slot * 6 + lane] = sr[lane];
  __syncthreads();
  if (lane == 0) {
    double d2 = __builtin_nan("");
    if (ok && chol6(sW)) {
      chol6_solve(sW, sy, 1);
      d2 = 0.0;
      for (int a = 0; a < 6; ++a) d2 += sr[a] * sy[a];
    }
    out.d2[slot] = d2;
  }
}

}  // namespace

void launch_pgcov_batch(const PgDev &p, const double *Ldiag, int nb, int ncb, const double *poses,
                        const int *trow_ptr, const int *trow, const PgCovGroup *groups, int ng,
                        const double *cand_val, double *Zw, int bw, const PgCovOut &out, hipStream_t s) {
  if (ng <= 0) return;
  (void)hipMemsetAsync(Zw, 0, (size_t)p.npad * bw * sizeof(double), s);
  hipLaunchKernelGGL(k_pgcov_rhs, dim3(ng), dim3(64), 0, s, groups, Zw, bw, p.pose_col);
  if (nb == 32)
    hipLaunchKernelGGL(k_pgcov_solve<32>, dim3(ng), dim3(64), 0, s, p.L, p.ld, Ldiag, ncb, trow_ptr, trow, groups,
                       Zw, bw, poses, cand_val, out);
  else
    hipLaunchKernelGGL(k_pgcov_solve<64>, dim3(ng), dim3(64), 0, s, p.L, p.ld, Ldiag, ncb, trow_ptr, trow, groups,
                       Zw, bw, poses, cand_val, out);
}

}  // namespace ba
