// ba_rel.hip — relative-pose factors on the handle path (ba_set_relative): loop closures and
// odometry edges between the poses of a resident problem.  The factor is defined once, in
// ba_rel_fn.h: r = se3_log(T_j T_k^-1 Z^-1), Jacobians I and
// -Ad(T_j T_k^-1); here its blocks live in a 126-double scratch record per factor.  Three
// kernels, launched only for a handle that holds factors, in a code object of their own:
//   k_rel_lin      per factor: the norm at the `sel` poses, optionally the linearisation
//                  into the scratch of that block buffer and the model's cross term
//   k_rel_gather   one thread per element of A_j / a_j walks the pose's list; workgroup 0
//                  adds the norm / cross-term partials to the exchange scalars
//   k_rel_offdiag  one thread per element of every coupled block walks the block's list and
//                  adds -Omega Ad to the packed S (and to the dense image)
// One writer per element, lists in input order, fixed trees: the same bits run to run.
#include "ba_handle.h"
#include "ba_rel_fn.h"

namespace ba {
namespace {

constexpr int kRelBlock = 256;
inline int rel_cdiv(int64_t a, int b) { return (int)((a + b - 1) / b); }

__global__ __launch_bounds__(kRelBlock) void k_rel_lin(DevProblem d, RelDev r, int sel, int mode) {
  __shared__ double sm[8];
  if (d.ctrl->done) return;
  const int buf = sel ? d.ctrl->tcur : d.ctrl->cur;
  const int lb = sel ? d.ctrl->tlcur : d.ctrl->lcur;
  const int lacc = d.ctrl->lcur;
  const double *P = d.poses[buf];
  const int f0 = blockIdx.x * kRelFpb;
  const int nf = min(kRelFpb, r.F - f0);
  const int tid = threadIdx.x;
  double *scr = r.scr[lb] + (size_t)f0 * kRelScr;
  const double *val = r.val + (size_t)f0 * 48;
  double cost = 0.0, cross = 0.0;
  if (tid < nf) {
    const int4 jk = r.jk[f0 + tid];
    if ((mode & 2) && jk.z >= 0 && jk.w >= 0)  // 2 x_j^T H_jk x_k with H_jk = -Omega Ad of the accepted point
      cross = rel_cross(r.scr[lacc] + (size_t)(f0 + tid) * kRelScr + kRelOA, d.x + (size_t)jk.z * 6,
                        d.x + (size_t)jk.w * 6);
    double RE[9], tE[3], rr[6];
    rel_E(jk, P, RE, tE);
    const double *Z = val + (size_t)tid * 48, *Om = Z + 12;
    rel_log(RE, tE, Z, rr);
    cost = sqrt(fmax(0.0, factor_quad<6>(Om, rr)));
    if (mode & 1) {  // r and Ad
      double *s = scr + (size_t)tid * kRelScr;
      rel_Ad(RE, tE, s + kRelAd);
#pragma unroll
      for (int a = 0; a < 6; ++a) s[kRelR + a] = rr[a];
    }
  }
  if (mode & 1) {
    __syncthreads();
    // OA = Omega Ad and Or = Omega r, one thread per element
    for (int e = tid; e < 42 * nf; e += kRelBlock) {
      const int f = e / 42, q = e - 42 * f;
      const double *Om = val + (size_t)f * 48 + 12;
      double *s = scr + (size_t)f * kRelScr;
      if (q < 36)
        s[kRelOA + q] = factor_OA<6>(Om, s + kRelAd, q);
      else
        s[kRelOr + q - 36] = factor_Or<6>(Om, s + kRelR, q - 36);
    }
    __syncthreads();
    // Bk = Ad^T OA and gk = Ad^T Or, for the factors whose k is optimisable
    for (int e = tid; e < 42 * nf; e += kRelBlock) {
      const int f = e / 42, q = e - 42 * f;
      if (r.jk[f0 + f].w < 0) continue;
      double *s = scr + (size_t)f * kRelScr;
      if (q < 36)
        s[kRelBk + q] = factor_Bk<6>(s + kRelAd, s + kRelOA, q);
      else
        s[kRelGk + q - 36] = factor_gk<6>(s + kRelAd, s + kRelOr, q - 36);
    }
  }
  block_sum2(cost, cross, sm);
  if (tid == 0) {
    r.part[2 * blockIdx.x + 0] = cost;
    r.part[2 * blockIdx.x + 1] = cross;
  }
}

__global__ __launch_bounds__(kRelBlock) void k_rel_gather(DevProblem d, RelDev r, int sel, int flags) {
  __shared__ double sm[8];
  if (d.ctrl->done) return;
  const int lb = sel ? d.ctrl->tlcur : d.ctrl->lcur;
  const int e = blockIdx.x * kRelBlock + threadIdx.x;
  if ((flags & 1) && e < 42 * d.N) {
    const int j = e / 42, q = e - 42 * j;
    const int l0 = r.pptr[j], l1 = r.pptr[j + 1];
    if (l0 < l1) {  // (a pose without a factor keeps its bits)
      bool any = false;
      const double acc = rel_walk_pose(r.val + 12, 48, r.scr[lb], r.plist, l0, l1, q, RelNoSkip{}, &any);
      if (q < 36)
        d.A[lb][(size_t)j * 36 + q] += acc;
      else
        d.a[lb][(size_t)j * 6 + q - 36] += acc;
    }
  }
  if (blockIdx.x != 0 || !(flags & 6)) return;
  double c = 0.0, x = 0.0;
  for (int k = threadIdx.x; k < r.n_part; k += kRelBlock) {
    c += r.part[2 * k + 0];
    x += r.part[2 * k + 1];
  }
  block_sum2(c, x, sm);
  if (threadIdx.x == 0) {
    if (flags & 2) d.scal[0] += c;
    if (flags & 4) d.scal[1] += x;
  }
}

__global__ __launch_bounds__(kRelBlock) void k_rel_offdiag(DevProblem d, RelDev r, int direct) {
  if (d.ctrl->done) return;
  const int e = blockIdx.x * kRelBlock + threadIdx.x;
  if (e >= 36 * r.nblk) return;
  const int b = e / 36, rc = e - 36 * b, rw = rc / 6, c = rc - 6 * rw;
  const int blk = r.blk[b];
  bool any = false;  // (a coupled block has a factor: unread)
  const double acc = rel_walk_block(r.scr[d.ctrl->lcur], r.blist, r.bptr[b], r.bptr[b + 1], rw, c, RelNoSkip{}, &any);
  d.Spk[(size_t)blk * 36 + rc] += acc;
  if (direct) {  // k_scatter's placement: a coupled block is never a diagonal one
    const int j = d.sblk_j[blk], k = d.sblk_k[blk];
    int row = d.pose_col[k] + c, col = d.pose_col[j] + rw;
    if (row < col) {
      const int t2 = row;
      row = col;
      col = t2;
    }
    d.L[(size_t)col * d.ld + row] += acc;
  }
}

}  // namespace

void launch_rel_lin(const DevProblem &d, const RelDev &r, int sel, int mode, hipStream_t s) {
  if (r.F <= 0) return;
  BA_LAUNCH(K_REL_LIN, k_rel_lin, dim3(r.n_part), dim3(kRelBlock), s, d, r, sel, mode);
}

void launch_rel_gather(const DevProblem &d, const RelDev &r, int sel, int flags, hipStream_t s) {
  if (r.F <= 0) return;
  const int grid = (flags & 1) ? rel_cdiv((int64_t)42 * d.N, kRelBlock) : 1;
  BA_LAUNCH(K_REL_GATHER, k_rel_gather, dim3(grid), dim3(kRelBlock), s, d, r, sel, flags);
}

void launch_rel_offdiag(const DevProblem &d, const RelDev &r, bool direct, hipStream_t s) {
  if (r.F <= 0 || r.nblk <= 0) return;
  BA_LAUNCH(K_REL_OFFDIAG, k_rel_offdiag, dim3(rel_cdiv((int64_t)36 * r.nblk, kRelBlock)), dim3(kRelBlock), s, d, r,
            direct ? 1 : 0);
}

}  // namespace ba
