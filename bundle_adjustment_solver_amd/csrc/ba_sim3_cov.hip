// ba_sim3_cov.hip — covariance blocks of a Sim(3) pose graph and the 7-DoF chi-square gate for
// loop-closure candidates (ba_sim3_covariance / ba_sim3_gate, include/ba_hip.h):
// ba_pgraph_cov.hip at seven columns per pose.
//
// With H = L L^T the tile Cholesky that dense_factor_solve leaves in the graph's dense image at
// lambda = 0, Sigma = H^-1 and Z_j = L^-1 E_j (the seven identity columns of pose j):
//   Sigma_jj = Z_j^T Z_j,   Sigma_jk = Z_j^T Z_k.
// One wave owns 16 right-hand sides: the columns of one pose in 0..6, of a second in 7..13;
// columns 14 and 15 stay zero.  It sweeps them with cov_sweep<NB> (ba_cov_sweep.h, unchanged), and
// its 16x16 Gram matrix holds Sigma_jj (rows and columns 0..6), Sigma_kk (7..13) and Sigma_jk
// between them.  What the wave does with them is the epilogue, through LDS:
//   kind 0 (two selected poses)  the two diagonal blocks
//   kind 1 (a pair j, k)         Sigma_jk (if asked for) and, with E = S_j S_k^-1 at the current
//                                poses and Ad = Ad7(E) (sim3_E / sim3_Ad of ba_sim3_fn.h),
//                                Sigma_E = Sigma_jj - Sigma_jk Ad^T - Ad Sigma_kj + Ad Sigma_kk Ad^T
//   kind 2 (a candidate)         also r = sim3_log(E Z^-1) (sim3_res), P = Sigma_E + Omega_z^-1 and
//                                d2 = r^T P^-1 r: two 7x7 Cholesky solves in plain fp64; a pivot of
//                                P that is not positive gives d2 = NaN
// A fixed member of a pair has no column: its blocks of the Gram matrix are exactly zero and the
// formula above is the reduced one.  No atomics, one writer per element, every sum in a fixed
// order: a block has the same bits run to run, in any selection and any batch split.
#include "ba_cov_sweep.h"
#include "ba_device.h"
#include "ba_device_fn.h"
#include "ba_sim3_host.h"
#include "ba_sim3_fn.h"

namespace ba {

namespace {

// identity columns of the group's optimisable members into the (zeroed) workspace
__global__ __launch_bounds__(64) void k_s3cov_rhs(const PgCovGroup *__restrict__ groups, double *Zw, int bw,
                                                  const int *__restrict__ pose_col) {
  const int lane = threadIdx.x;
  if (lane >= 14) return;
  const int a = lane / 7, r = lane - 7 * a;
  const int j = groups[blockIdx.x].opt[a];
  if (j >= 0) Zw[(size_t)(pose_col[j] + r) * bw + kCovGroupCols * blockIdx.x + 7 * a + r] = 1.0;
}

// In-place Cholesky of the 7x7 matrix A (row-major, LDS; the lower triangle is read and
// replaced by the factor); false at a pivot that is not positive.  One lane.
__device__ __forceinline__ bool chol7(double *A) {
  for (int c = 0; c < 7; ++c) {
    double d = A[c * 7 + c];
    for (int m = 0; m < c; ++m) d -= A[c * 7 + m] * A[c * 7 + m];
    if (!(d > 0.0)) return false;
    const double s = sqrt(d);
    A[c * 7 + c] = s;
    for (int r = c + 1; r < 7; ++r) {
      double v = A[r * 7 + c];
      for (int m = 0; m < c; ++m) v -= A[r * 7 + m] * A[c * 7 + m];
      A[r * 7 + c] = v / s;
    }
  }
  return true;
}
// x <- (L L^T)^-1 x for the factor chol7 left in A (x: 7 doubles in LDS, stride xs).  One lane.
__device__ __forceinline__ void chol7_solve(const double *A, double *x, const int xs) {
  for (int r = 0; r < 7; ++r) {
    double v = x[r * xs];
    for (int m = 0; m < r; ++m) v -= A[r * 7 + m] * x[m * xs];
    x[r * xs] = v / A[r * 7 + r];
  }
  for (int r = 6; r >= 0; --r) {
    double v = x[r * xs];
    for (int m = r + 1; m < 7; ++m) v -= A[m * 7 + r] * x[m * xs];
    x[r * xs] = v / A[r * 7 + r];
  }
}

template <int NB>
__global__ __launch_bounds__(64) void k_s3cov_solve(const double *__restrict__ L, int ld,
                                                    const double *__restrict__ Ldiag, int ncb,
                                                    const int *__restrict__ trow_ptr,
                                                    const int *__restrict__ trow,
                                                    const PgCovGroup *__restrict__ groups, double *Zw, int bw,
                                                    const double *__restrict__ poses,
                                                    const double *__restrict__ cand_val, S3CovOut out) {
  __shared__ double sG[256];                       // the Gram matrix, row-major
  __shared__ double sAd[49], sA[49], sS[49], sW[49], sP[49], sr[7], sy[7];
  __shared__ int ok;
  const PgCovGroup g = groups[blockIdx.x];
  const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4;
  double *Zc = Zw + kCovGroupCols * blockIdx.x + lr;  // this lane's column
  const cov_v4f64 G = cov_sweep<NB>(L, ld, Ldiag, ncb, trow_ptr, trow, g.t0, Zc, bw);
#pragma unroll
  for (int q = 0; q < 4; ++q) sG[(lk + 4 * q) * 16 + lr] = G[q];
  __syncthreads();
  if (g.kind == kPgCovPoses) {  // the diagonal blocks
    for (int e = lane; e < 98; e += 64) {
      const int a = e / 49, q = e - 49 * a, r = q / 7, c = q - 7 * r;
      if (g.slot[a] >= 0) out.pose49[(size_t)g.slot[a] * 49 + q] = sG[(7 * a + r) * 16 + 7 * a + c];
    }
    return;
  }
  const size_t slot = (size_t)g.slot[0];
  // a candidate's Z (13) and Omega_z (49, mirrored by the host)
  const double *val = g.kind == kPgCovCand ? cand_val + slot * kS3Val : nullptr;
  if (lane == 0) {
    double E[13];
    sim3_E(g.pose[0], g.pose[1], poses, E);
    sim3_Ad(E, sAd);
    if (g.kind == kPgCovCand) {
      double rr[7];
      sim3_res(E, val, rr);
#pragma unroll
      for (int a = 0; a < 7; ++a) sr[a] = sy[a] = rr[a];
    }
  }
  __syncthreads();
  const int r0 = lane / 7, c0 = lane - 7 * r0;  // lanes 0..48: one element of a 7x7 block each
  if (lane < 49) {  // A = Ad Sigma_kk
    double acc = 0.0;
    for (int m = 0; m < 7; ++m) acc += sAd[r0 * 7 + m] * sG[(7 + m) * 16 + 7 + c0];
    sA[lane] = acc;
  }
  __syncthreads();
  if (lane < 49) {
    // element (r0, c0) of Sigma_E from the expression of its lower-triangle twin, so that the
    // block is symmetric to the bit (Sigma_kj[m][c] = Sigma_jk[c][m], the Gram matrix is)
    const int a = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
    double t1 = 0.0, t2 = 0.0, t3 = 0.0;
    for (int m = 0; m < 7; ++m) {
      t1 += sG[a * 16 + 7 + m] * sAd[c * 7 + m];
      t2 += sAd[a * 7 + m] * sG[c * 16 + 7 + m];
      t3 += sA[a * 7 + m] * sAd[c * 7 + m];
    }
    const double v = ((sG[a * 16 + c] - t1) - t2) + t3;
    sS[lane] = v;
    out.rel49[slot * 49 + lane] = v;
    if (out.cross49) out.cross49[slot * 49 + lane] = sG[r0 * 16 + 7 + c0];
    if (g.kind == kPgCovCand) sW[lane] = val[13 + lane];
  }
  if (g.kind != kPgCovCand) return;
  __syncthreads();
  // Omega_z^-1: the factor once, then one solve per identity column (lanes 0..6), in sP
  if (lane == 0) ok = chol7(sW) ? 1 : 0;
  if (lane < 49) sP[lane] = r0 == c0 ? 1.0 : 0.0;
  __syncthreads();
  if (lane < 7 && ok) chol7_solve(sW, sP + lane, 7);
  __syncthreads();
  double pv = 0.0;
  if (lane < 49) {  // P = Sigma_E + Omega_z^-1, the inverse read from its lower-triangle twin
    const int a = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
    pv = sS[lane] + sP[a * 7 + c];
  }
  __syncthreads();
  if (lane < 49) {
    sW[lane] = pv;
    if (out.innov49) out.innov49[slot * 49 + lane] = ok ? pv : __builtin_nan("");
  }
  if (lane < 7 && out.r7) out.r7[slot * 7 + lane] = sr[lane];
  __syncthreads();
  if (lane == 0) {
    double d2 = __builtin_nan("");
    if (ok && chol7(sW)) {
      chol7_solve(sW, sy, 1);
      d2 = 0.0;
      for (int a = 0; a < 7; ++a) d2 += sr[a] * sy[a];
    }
    out.d2[slot] = d2;
  }
}

}  // namespace

void launch_s3cov_batch(const PgDev &p, const double *Ldiag, int nb, int ncb, const double *poses,
                        const int *trow_ptr, const int *trow, const PgCovGroup *groups, int ng,
                        const double *cand_val, double *Zw, int bw, const S3CovOut &out, hipStream_t s) {
  if (ng <= 0) return;
  (void)hipMemsetAsync(Zw, 0, (size_t)p.npad * bw * sizeof(double), s);
  hipLaunchKernelGGL(k_s3cov_rhs, dim3(ng), dim3(64), 0, s, groups, Zw, bw, p.pose_col);
  if (nb == 32)
    hipLaunchKernelGGL(k_s3cov_solve<32>, dim3(ng), dim3(64), 0, s, p.L, p.ld, Ldiag, ncb, trow_ptr, trow, groups,
                       Zw, bw, poses, cand_val, out);
  else
    hipLaunchKernelGGL(k_s3cov_solve<64>, dim3(ng), dim3(64), 0, s, p.L, p.ld, Ldiag, ncb, trow_ptr, trow, groups,
                       Zw, bw, poses, cand_val, out);
}

}  // namespace ba
