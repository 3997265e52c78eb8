// ba_rel_fn.h — the relative-pose factor on the device, once: the handle path
// (ba_rel.hip), the batch path (ba_batch_kernels.h) and the pose graph (ba_pgraph.hip) call
// these functions and differ only in where a factor's blocks live.  Factor f between the
// poses j and k: r = se3_log(T_j T_k^-1 Z^-1), first-order Jacobians dr/dxi_j = I and
// dr/dxi_k = -Ad(T_j T_k^-1), so that with Omega mirrored by the host
//   H_jj += Omega         g_j += -Omega r          H_jk += -Omega Ad
//   H_kk += Ad^T Omega Ad g_k += Ad^T Omega r
// Device only; every function is forced inline and the library builds with
// -ffp-contract=off, so that one expression gives the same bits in every caller.
#ifndef BA_REL_FN_H_
#define BA_REL_FN_H_

#include "ba_device_fn.h"
#include "ba_factor_fn.h"

namespace ba {

// scratch of one factor on the handle and batch paths (kRelScr doubles, ba_device.h), in
// doubles: r, Omega r, Ad^T Omega r, Ad, Omega Ad, Ad^T Omega Ad
constexpr int kRelR = 0, kRelOr = 6, kRelGk = 12, kRelAd = 18, kRelOA = 54, kRelBk = 90;
static_assert(kRelBk + 36 == kRelScr, "the record ends with Ad^T Omega Ad");

// E = T_j T_k^-1 = [RE, tE] of one factor at the poses P
__device__ __forceinline__ void rel_E(const int4 jk, const double *P, double RE[9], double tE[3]) {
  const double *Tj = P + jk.x * 12, *Tk = P + jk.y * 12;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c)  // R_j R_k^T
      RE[a * 3 + c] = Tj[a * 3 + 0] * Tk[c * 3 + 0] + Tj[a * 3 + 1] * Tk[c * 3 + 1] + Tj[a * 3 + 2] * Tk[c * 3 + 2];
#pragma unroll
  for (int a = 0; a < 3; ++a) tE[a] = Tj[9 + a] - (RE[a * 3 + 0] * Tk[9] + RE[a * 3 + 1] * Tk[10] + RE[a * 3 + 2] * Tk[11]);
}

// the residual r = se3_log(E Z^-1)
__device__ __forceinline__ void rel_log(const double RE[9], const double tE[3], const double *Z, double *r) {
  double RD[9], tD[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c)  // R_E R_Z^T
      RD[a * 3 + c] = RE[a * 3 + 0] * Z[c * 3 + 0] + RE[a * 3 + 1] * Z[c * 3 + 1] + RE[a * 3 + 2] * Z[c * 3 + 2];
#pragma unroll
  for (int a = 0; a < 3; ++a) tD[a] = tE[a] - (RD[a * 3 + 0] * Z[9] + RD[a * 3 + 1] * Z[10] + RD[a * 3 + 2] * Z[11]);
  se3_log(RD, tD, r);
}

// Ad = [[R_E, [t_E]x R_E], [0, R_E]] as 36 doubles, row-major (global scratch or an LDS row)
__device__ __forceinline__ void rel_Ad(const double RE[9], const double tE[3], double *Ad) {
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
}

// (r^T Omega r and the elements of Omega Ad, Omega r, Ad^T Omega Ad, Ad^T Omega r that the
// per-element threads take are factor_quad / factor_OA / factor_Or / factor_Bk / factor_gk of
// ba_factor_fn.h at width 6; factor_Bk holds the rule that keeps Ad^T Omega Ad symmetric to the bit)

// the cross term 2 x_j^T H_jk x_k = -2 x_j^T OA x_k of the quadratic model
__device__ __forceinline__ double rel_cross(const double *OA, const double *xj, const double *xk) {
  double q = 0.0;
  for (int a = 0; a < 6; ++a) {
    double row = 0.0;
    for (int c = 0; c < 6; ++c) row += OA[a * 6 + c] * xk[c];
    q += xj[a] * row;
  }
  return -2.0 * q;
}

// The two list walks of the handle and batch paths, whose factors keep the kRelScr record in scr and
// Omega (36 per factor) every om_s doubles of Om.  skip(f): the factor does not join; *any: one did.
// (k_graph_assemble keeps both written out, its own record and the robust weight in them: these measured slower.)
// Element q < 42 of {H_jj, g_j} of one optimisable pose: its list entries [l0, l1)
// (factor << 1 | (1: it is the factor's k)) in input order.
template <class Skip>
__device__ __forceinline__ double rel_walk_pose(const double *Om, const int om_s, const double *scr,
                                                const int32_t *plist, const int l0, const int l1, const int q,
                                                Skip skip, bool *any) {
  double acc = 0.0;
  for (int l = l0; l < l1; ++l) {
    const int w = plist[l], f = w >> 1;
    if (skip(f)) continue;
    *any = true;
    const double *s = scr + (size_t)f * kRelScr;
    if (q < 36)
      acc += (w & 1) ? s[kRelBk + q] : Om[(size_t)f * om_s + q];
    else
      acc += (w & 1) ? s[kRelGk + q - 36] : -s[kRelOr + q - 36];
  }
  return acc;
}
// Element (r, c) of H_hi,lo = sum -OA (or -OA^T) of one coupled block: its list entries
// [l0, l1) (factor << 1 | (1: H_jk lies transposed)) in input order.
template <class Skip>
__device__ __forceinline__ double rel_walk_block(const double *scr, const int32_t *blist, const int l0, const int l1,
                                                 const int r, const int c, Skip skip, bool *any) {
  double acc = 0.0;
  for (int l = l0; l < l1; ++l) {
    const int w = blist[l], f = w >> 1;
    if (skip(f)) continue;
    *any = true;
    acc -= scr[(size_t)f * kRelScr + kRelOA + ((w & 1) ? c * 6 + r : r * 6 + c)];
  }
  return acc;
}
struct RelNoSkip {  // every factor joins
  __device__ __forceinline__ bool operator()(int) const { return false; }
};

}  // namespace ba
#endif  // BA_REL_FN_H_
