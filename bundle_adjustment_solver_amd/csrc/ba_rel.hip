// ba_rel.hip — relative-pose factors on the handle path (ba_set_relative): loop closures and
// odometry edges between the poses of a resident problem.  The definition is the batch
// path's (ba_batch_kernels.h): r = se3_log(T_j T_k^-1 Z^-1), Jacobians I and
// -Ad(T_j T_k^-1), the 126-double scratch record per factor.  Three kernels, launched only
// for a handle that holds factors, in a code object of their own:
//   k_rel_lin      per factor: the norm at the `sel` poses, optionally the linearisation
//                  into the scratch of that block buffer and the model's cross term
//   k_rel_gather   one thread per element of A_j / a_j walks the pose's list; workgroup 0
//                  adds the norm / cross-term partials to the exchange scalars
//   k_rel_offdiag  one thread per element of every coupled block walks the block's list and
//                  adds -Omega Ad to the packed S (and to the dense image)
// One writer per element, lists in input order, fixed trees: the same bits run to run.
#include "ba_batch_kernels.h"

namespace ba {
namespace {

constexpr int kRelBlock = 256;
static_assert(kRelScr == kRelScrDoubles, "the host sizes the scratch by the batch path's record");
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
    if ((mode & 2) && jk.z >= 0 && jk.w >= 0) {
      // 2 x_j^T H_jk x_k with H_jk = -Omega Ad of the accepted point
      const double *OA = r.scr[lacc] + (size_t)(f0 + tid) * kRelScr + kRelOA;
      const double *xj = d.x + (size_t)jk.z * 6, *xk = d.x + (size_t)jk.w * 6;
      double q = 0.0;
      for (int a = 0; a < 6; ++a) {
        double row = 0.0;
        for (int c = 0; c < 6; ++c) row += OA[a * 6 + c] * xk[c];
        q += xj[a] * row;
      }
      cross = -2.0 * q;
    }
    double RE[9], tE[3], rr[6];
    rel_E(jk, P, RE, tE);
    const double *Z = val + (size_t)tid * 48, *Om = Z + 12;
    rel_log(RE, tE, Z, rr);
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      double row = 0.0;
#pragma unroll
      for (int c = 0; c < 6; ++c) row += Om[a * 6 + c] * rr[c];
      q += rr[a] * row;
    }
    cost = sqrt(fmax(0.0, q));
    if (mode & 1) {  // r and Ad = [[R_E, [t_E]x R_E], [0, R_E]]
      double *s = scr + (size_t)tid * kRelScr;
      double *Ad = s + kRelAd;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Ad[0 * 6 + 3 + c] = tE[1] * RE[6 + c] - tE[2] * RE[3 + c];
        Ad[1 * 6 + 3 + c] = tE[2] * RE[0 + c] - tE[0] * RE[6 + c];
        Ad[2 * 6 + 3 + c] = tE[0] * RE[3 + c] - tE[1] * RE[0 + c];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          Ad[a * 6 + c] = RE[a * 3 + c];
          Ad[(3 + a) * 6 + 3 + c] = RE[a * 3 + c];
          Ad[(3 + a) * 6 + c] = 0.0;
        }
      }
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
      double acc = 0.0;
      if (q < 36) {
        const int a = q / 6, c = q - 6 * a;
        for (int m = 0; m < 6; ++m) acc += Om[a * 6 + m] * s[kRelAd + m * 6 + c];
        s[kRelOA + q] = acc;
      } else {
        const int a = q - 36;
        for (int m = 0; m < 6; ++m) acc += Om[a * 6 + m] * s[kRelR + m];
        s[kRelOr + a] = acc;
      }
    }
    __syncthreads();
    // Bk = Ad^T OA (each element from the expression of its lower-triangle twin: symmetric to
    // the bit) and gk = Ad^T Or, for the factors whose k is optimisable
    for (int e = tid; e < 42 * nf; e += kRelBlock) {
      const int f = e / 42, q = e - 42 * f;
      if (r.jk[f0 + f].w < 0) continue;
      double *s = scr + (size_t)f * kRelScr;
      double acc = 0.0;
      if (q < 36) {
        const int r0 = q / 6, c0 = q - 6 * r0;
        const int a = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
        for (int m = 0; m < 6; ++m) acc += s[kRelAd + m * 6 + a] * s[kRelOA + m * 6 + c];
        s[kRelBk + q] = acc;
      } else {
        const int a = q - 36;
        for (int m = 0; m < 6; ++m) acc += s[kRelAd + m * 6 + a] * s[kRelOr + m];
        s[kRelGk + a] = acc;
      }
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
      const double *scr = r.scr[lb];
      double acc = 0.0;
      for (int l = l0; l < l1; ++l) {
        const int w = r.plist[l], f = w >> 1;
        const double *s = scr + (size_t)f * kRelScr;
        if (q < 36)
          acc += (w & 1) ? s[kRelBk + q] : r.val[(size_t)f * 48 + 12 + q];
        else
          acc += (w & 1) ? s[kRelGk + q - 36] : -s[kRelOr + q - 36];
      }
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
  const double *scr = r.scr[d.ctrl->lcur];
  const int l1 = r.bptr[b + 1];
  double acc = 0.0;
  for (int l = r.bptr[b]; l < l1; ++l) {
    const int w = r.blist[l], f = w >> 1;
    acc -= scr[(size_t)f * kRelScr + kRelOA + ((w & 1) ? c * 6 + rw : rc)];
  }
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
