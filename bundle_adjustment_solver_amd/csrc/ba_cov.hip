// ba_cov.hip — covariance blocks from the factored reduced camera system (ba_covariance).
//
// The reference has no counterpart.  With S = L L^T the tile Cholesky that
// dense_factor_solve leaves in the dense image (off-diagonal tiles in d.L, the factor
// and the 16x16 tile inverses of the diagonal tiles in d.Ldiag), at lambda = 0:
//   pose block      [S^-1]_jj = Z_j^T Z_j,            Z_j = L^-1 E_j   (6 identity columns)
//   landmark block  Sigma_ii  = Cinv_i + U_i^T U_i,   U_i = L^-1 (sum_j E_j W_ji Cinv_i)
// (U_i = sum_j Z_j (W_ji Cinv_i) by linearity: three right-hand sides per landmark, which
// carry every pose block of S^-1 the landmark needs, off-diagonal ones included, and
// nothing has to be accumulated across column batches.)
//
// One wave owns 16 right-hand sides — two poses or five landmarks — and sweeps the row
// tiles of the image top to bottom (left-looking):
//   R_t = E_t - sum_{s < t, L(t,s) != 0} L(t,s) X_s      v_mfma_f64_16x16x4_f64
//   X_t = L_tt^-1 R_t                                     block forward substitution with
//                                                         the stored tile inverses, MFMA
//   G  += X_t^T X_t                                       the 16x16 Gram matrix, MFMA
// X_t goes to the wave's 16 columns of the workspace (row-major, npad x batch columns),
// which only this wave reads back.  Rows above the first non-zero row of the group's
// right-hand sides are zero and skipped; structurally zero tiles of the factor are
// skipped through the schedule's row lists.  The diagonal blocks of G are the results.
// No atomics; every sum is an MFMA chain in tile order: the same bits run to run and
// whatever else is selected in the same call.
#include "ba_cov_sweep.h"
#include "ba_device.h"
#include "ba_device_fn.h"

namespace ba {

namespace {
typedef cov_v4f64 v4f64;

// Right-hand sides of the batch into the (zeroed) workspace: identity columns of the
// group's poses, or W_ji Cinv_i (6x3, W expanded from the compact {K, X_ij} record as
// ba_get_pairs does) in the rows of pose j for every pair of the group's landmarks.  The
// pairs below P_slim hold {G, w} (ba_device.h kWSlim): {K, X_ij} by pair_from_G, from the
// poses and points of the linearisation.
__global__ __launch_bounds__(64) void k_cov_rhs(const CovGroup *__restrict__ groups, double *Zw, int bw,
                                                const int *__restrict__ pose_col,
                                                const int64_t *__restrict__ lm_pair_ptr,
                                                const int32_t *__restrict__ pair_pose,
                                                const double *__restrict__ W,
                                                const double *__restrict__ Cinv, const int64_t P_slim,
                                                const double *__restrict__ poses,
                                                const double *__restrict__ pts) {
  const CovGroup g = groups[blockIdx.x];
  const int lane = threadIdx.x;
  const int cb = kCovGroupCols * blockIdx.x;
  if (g.kind == 0) {
    const int a = lane / 6, r = lane % 6;
    if (a < g.n) Zw[(size_t)(pose_col[g.item[a]] + r) * bw + cb + 6 * a + r] = 1.0;
    return;
  }
  for (int a = 0; a < g.n; ++a) {
    const int i = g.item[a];
    const double *ci = Cinv + (size_t)i * 6;
    const double c00 = ci[0], c01 = ci[1], c02 = ci[2], c11 = ci[3], c12 = ci[4], c22 = ci[5];
    for (int64_t p = lm_pair_ptr[i] + lane; p < lm_pair_ptr[i + 1]; p += 64) {
      const double *k = W + (size_t)p * kWStride;
      double k12[12];
      if (p < P_slim) {
        const double *rec = W + (size_t)p * kWSlim;
        const double G[6] = {rec[0], rec[1], rec[2], rec[3], rec[4], rec[5]};
        const double *X = pts + (size_t)i * 3;
        pair_from_G(G, rec[6], poses + (size_t)pair_pose[p] * 12, X[0], X[1], X[2], k12, k12 + 9);
        k = k12;
      }
      double w[6][3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        w[0][c] = k[c];
        w[1][c] = k[3 + c];
        w[2][c] = k[6 + c];
        w[3][c] = k[10] * k[6 + c] - k[11] * k[3 + c];
        w[4][c] = k[11] * k[c] - k[9] * k[6 + c];
        w[5][c] = k[9] * k[3 + c] - k[10] * k[c];
      }
      double *dst = Zw + (size_t)pose_col[pair_pose[p]] * bw + cb + 3 * a;
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        dst[(size_t)r * bw + 0] = w[r][0] * c00 + w[r][1] * c01 + w[r][2] * c02;
        dst[(size_t)r * bw + 1] = w[r][0] * c01 + w[r][1] * c11 + w[r][2] * c12;
        dst[(size_t)r * bw + 2] = w[r][0] * c02 + w[r][1] * c12 + w[r][2] * c22;
      }
    }
  }
}

// The sweep itself is cov_sweep<NB> (ba_cov_sweep.h), shared with the pose graph's kernel; an
// accumulator register q of the Gram matrix is G[row = lk + 4 q][column = lr].
template <int NB>
__global__ __launch_bounds__(64) void k_cov_solve(const double *__restrict__ L, int ld,
                                                  const double *__restrict__ Ldiag, int ncb,
                                                  const int *__restrict__ trow_ptr,
                                                  const int *__restrict__ trow,
                                                  const CovGroup *__restrict__ groups, double *Zw,
                                                  int bw, const double *__restrict__ Cinv,
                                                  double *out_pose, double *out_pt) {
  const CovGroup g = groups[blockIdx.x];
  const int lane = threadIdx.x, lr = lane & 15, lk = lane >> 4;
  double *Zc = Zw + kCovGroupCols * blockIdx.x + lr;  // this lane's column
  const v4f64 G = cov_sweep<NB>(L, ld, Ldiag, ncb, trow_ptr, trow, g.t0, Zc, bw);
  // the diagonal blocks of G: 6x6 per pose, or Cinv_i + 3x3 per landmark
  const int bs = g.kind == 0 ? 6 : 3;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int row = lk + 4 * q, a = row / bs;
    if (a >= g.n || lr / bs != a) continue;
    const int r = row - bs * a, c = lr - bs * a;
    if (g.kind == 0) {
      out_pose[(size_t)g.slot[a] * 36 + 6 * r + c] = G[q];
    } else {
      const int lo = r < c ? r : c, hi = r < c ? c : r;
      const int sym = lo == 0 ? hi : lo + hi + 1;  // (00 01 02 11 12 22)
      out_pt[(size_t)g.slot[a] * 9 + 3 * r + c] = Cinv[(size_t)g.item[a] * 6 + sym] + G[q];
    }
  }
}

}  // namespace

void launch_cov_batch(const DevProblem &d, int lcur, int cur, int ncb, const int *trow_ptr, const int *trow,
                      const CovGroup *groups, int ng, double *Zw, int bw, double *out_pose,
                      double *out_pt, hipStream_t s) {
  if (ng <= 0) return;
  (void)hipMemsetAsync(Zw, 0, (size_t)d.npad * bw * sizeof(double), s);
  hipLaunchKernelGGL(k_cov_rhs, dim3(ng), dim3(64), 0, s, groups, Zw, bw, d.pose_col, d.lm_pair_ptr,
                     d.pair_pose, d.W[lcur], d.Cinv, d.P_slim, d.poses[cur], d.pts[cur]);
  if (d.nb == 32)
    hipLaunchKernelGGL(k_cov_solve<32>, dim3(ng), dim3(64), 0, s, d.L, d.ld, d.Ldiag, ncb, trow_ptr, trow,
                       groups, Zw, bw, d.Cinv, out_pose, out_pt);
  else
    hipLaunchKernelGGL(k_cov_solve<64>, dim3(ng), dim3(64), 0, s, d.L, d.ld, d.Ldiag, ncb, trow_ptr, trow,
                       groups, Zw, bw, d.Cinv, out_pose, out_pt);
}

}  // namespace ba
