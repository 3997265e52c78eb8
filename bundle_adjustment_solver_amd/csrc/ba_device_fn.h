// ba_device_fn.h — __device__ building blocks shared by the kernels of the handle path
// (ba_kernels.hip) and the batched full-BA kernel (ba_batch.hip): block reductions, the
// per-observation geometry of the linearisation, the 3x3 inverses, the se3 exponential
// and the trust-region control step.  Internal; every function is forced inline, so a
// kernel compiles exactly as if the function were written in its own file.
#ifndef BA_DEVICE_FN_H_
#define BA_DEVICE_FN_H_

#include "ba_device.h"

namespace ba {

// Wave-wide sum on the DPP network (no LDS round trips): xor-1, xor-2,
// half-mirror and mirror steps leave every lane with the total of its row of
// 16, the four row totals are then added in order.  Fixed association:
// deterministic; every lane returns the total.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  union { double d; int i[2]; } u, r;
  u.d = v;
  r.i[0] = __builtin_amdgcn_update_dpp(0, u.i[0], CTRL, 0xf, 0xf, false);
  r.i[1] = __builtin_amdgcn_update_dpp(0, u.i[1], CTRL, 0xf, 0xf, false);
  return r.d;
}
__device__ __forceinline__ double lane_f64(double v, int src) {
  union { double d; int i[2]; } u;
  u.d = v;
  u.i[0] = __builtin_amdgcn_readlane(u.i[0], src);
  u.i[1] = __builtin_amdgcn_readlane(u.i[1], src);
  return u.d;
}
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);  // row_half_mirror
  v += dpp_f64<0x140>(v);  // row_mirror
  return ((lane_f64(v, 0) + lane_f64(v, 16)) + lane_f64(v, 32)) + lane_f64(v, 48);
}

// Sum over a 256-thread block; result valid in thread 0.  `sm` holds >= 4.
__device__ __forceinline__ double block_sum(double v, double *sm) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sm[wv] = v;
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
    for (int w = 0; w < nw; ++w) r += sm[w];
  }
  return r;
}

// Two sums over a 256-thread block with one pair of barriers; valid in thread 0.
// `sm` holds >= 8.
__device__ __forceinline__ void block_sum2(double &a, double &b, double *sm) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
    sm[wv] = a;
    sm[4 + wv] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    b = ((sm[4] + sm[5]) + sm[6]) + sm[7];
  }
}

// The camera table (16 doubles per camera: fx fy cx cy, R_cj row-major, t_cj) of a
// problem with at most kCamLds cameras is staged in LDS by the kernels that gather it.
constexpr int kCamLds = 8;

// Projection of one observation; reference :743-760 / :413-425.
struct ObsGeom {
  double Xij[3];
  double Xc[3];
  double r0, r1;
};

__device__ __forceinline__ void project(const double *__restrict__ cam,
                                        const double *__restrict__ T,
                                        const double X0, const double X1,
                                        const double X2, const double u,
                                        const double v, ObsGeom &g) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int r = 0; r < 3; ++r)
    g.Xij[r] = (T[r * 3 + 0] * X0 + T[r * 3 + 1] * X1 + T[r * 3 + 2] * X2) +
               T[9 + r];
  const double *Rc = cam + 4;
  const double *tc = cam + 13;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    g.Xc[r] = (Rc[r * 3 + 0] * g.Xij[0] + Rc[r * 3 + 1] * g.Xij[1] +
               Rc[r * 3 + 2] * g.Xij[2]) +
              tc[r];
  const double invz = 1.0 / g.Xc[2];
  g.r0 = cam[0] * (g.Xc[0] * invz) + cam[2] - u;
  g.r1 = cam[1] * (g.Xc[1] * invz) + cam[3] - v;
}

// Huber-like weight (reference :763-766) and G = dpi/dXc * R_cj (:770-787).
__device__ __forceinline__ void weight_and_G(const double *__restrict__ cam,
                                             const ObsGeom &g, double huber,
                                             double &w, double G[6]) {
#pragma clang fp contract(fast)
  const double invz = 1.0 / g.Xc[2];
  const double fxinvz = cam[0] * invz, fyinvz = cam[1] * invz;
  const double xinvz = g.Xc[0] * invz, yinvz = g.Xc[1] * invz;
  const double fx_xinvz2 = fxinvz * xinvz, fy_yinvz2 = fyinvz * yinvz;
  const double absr = fabs(g.r0) + fabs(g.r1);
  w = (absr > huber) ? (huber / absr) : 1.0;
  const double *Rc = cam + 4;
  G[0] = fxinvz * Rc[0] + (-fx_xinvz2) * Rc[6];
  G[1] = fxinvz * Rc[1] + (-fx_xinvz2) * Rc[7];
  G[2] = fxinvz * Rc[2] + (-fx_xinvz2) * Rc[8];
  G[3] = fyinvz * Rc[3] + (-fy_yinvz2) * Rc[6];
  G[4] = fyinvz * Rc[4] + (-fy_yinvz2) * Rc[7];
  G[5] = fyinvz * Rc[5] + (-fy_yinvz2) * Rc[8];
}

// Q = [G, G * (-[Xij]x)]  (reference :797-800), 2x6 row-major
__device__ __forceinline__ void make_Q(const double G[6], const double Xij[3],
                                       double Q[12]) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const double g0 = G[r * 3 + 0], g1 = G[r * 3 + 1], g2 = G[r * 3 + 2];
    Q[r * 6 + 0] = g0;
    Q[r * 6 + 1] = g1;
    Q[r * 6 + 2] = g2;
    Q[r * 6 + 3] = g2 * Xij[1] - g1 * Xij[2];
    Q[r * 6 + 4] = g0 * Xij[2] - g2 * Xij[0];
    Q[r * 6 + 5] = g1 * Xij[0] - g0 * Xij[1];
  }
}

// R = G * R_jw (reference :814), 2x3 row-major
__device__ __forceinline__ void make_R(const double G[6],
                                       const double *__restrict__ T,
                                       double Rm[6]) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      Rm[r * 3 + c] = G[r * 3 + 0] * T[0 * 3 + c] + G[r * 3 + 1] * T[1 * 3 + c] +
                      G[r * 3 + 2] * T[2 * 3 + c];
}

// rows 3..5 of B_ji from its compact record {K (9), X_ij (3)}: row 3+a, column c
// = (X_ij x K[:,c])[a]
__device__ __forceinline__ void expand_W(const double *__restrict__ k12, double W[18]) {
#pragma unroll
  for (int e = 0; e < 9; ++e) W[e] = k12[e];
  const double X0 = k12[9], X1 = k12[10], X2 = k12[11];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    W[9 + c] = X1 * k12[6 + c] - X2 * k12[3 + c];
    W[12 + c] = X2 * k12[c] - X0 * k12[6 + c];
    W[15 + c] = X0 * k12[3 + c] - X1 * k12[c];
  }
}

// The compact record {K (9), X_ij (3)} of a pair from its slim one (ba_device.h kWSlim):
// G (2x3) and w of the pair's last writer, the pose T = {R_jw row-major, t_jw} and the
// point X_i.  K = G^T (w (G R_jw)), X_ij = R_jw X_i + t_jw — with the operations and the
// roundings of the writer's own expressions (project, make_R and the K of k_lin_grp as the
// compiler contracts them: a sum of products fuses its first product onto the rounded
// second, a further product is fused onto the sum, "+ t" is an addition of its own), spelled
// out with fma() so that no reader depends on a contraction setting: kernels and the host's
// block getter get the bits the 96-byte record holds.  A zero record (w = 0, G = 0: masked
// pair without an observation) gives K = 0 exactly.
__host__ __device__ __forceinline__ void pair_from_G(const double G[6], const double w, const double *__restrict__ T,
                                                     const double X0, const double X1, const double X2, double K[9],
                                                     double Xij[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < 3; ++r)
    Xij[r] = fma(T[r * 3 + 2], X2, fma(T[r * 3 + 0], X0, T[r * 3 + 1] * X1)) + T[9 + r];
  double wR[6];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      wR[m * 3 + c] = w * fma(G[m * 3 + 2], T[6 + c], fma(G[m * 3 + 0], T[c], G[m * 3 + 1] * T[3 + c]));
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) K[r * 3 + c] = fma(G[r], wR[c], G[3 + r] * wR[3 + c]);
}

// The slim record {G, w} of a pair from the observation of its last writer: what k_lin_grp
// computes for that observation through project() and weight_and_G(), with the operations
// and the roundings of the kernel's generated code (a sum of three products starts from the
// rounded MIDDLE product and fuses the first, then the third; "+ t" is an addition of its own;
// fx (x / z) + cx is one fma, "- u" a subtraction; a row of G fuses f / z * R onto the rounded
// product with R's third row; both divisions are IEEE divisions), spelled out with fma() like
// pair_from_G.  The readers of the "from the observation" record form (ba_device.h PairObs)
// call it in front of pair_from_G; the observation is a valid one (no masked slot).
__host__ __device__ __forceinline__ void pair_G_from_obs(const double *__restrict__ cam, const double *__restrict__ T,
                                                         const double X0, const double X1, const double X2,
                                                         const double u, const double v, const double huber,
                                                         double G[6], double &w) {
#pragma clang fp contract(off)
  double Xij[3], Xc[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    Xij[r] = fma(T[r * 3 + 2], X2, fma(T[r * 3 + 0], X0, T[r * 3 + 1] * X1)) + T[9 + r];
  const double *Rc = cam + 4;
#pragma unroll
  for (int r = 0; r < 3; ++r)
    Xc[r] = fma(Rc[r * 3 + 2], Xij[2], fma(Rc[r * 3 + 0], Xij[0], Rc[r * 3 + 1] * Xij[1])) + cam[13 + r];
  const double invz = 1.0 / Xc[2];
  const double xinvz = Xc[0] * invz, yinvz = Xc[1] * invz;
  const double r0 = fma(cam[0], xinvz, cam[2]) - u;
  const double r1 = fma(cam[1], yinvz, cam[3]) - v;
  const double absr = fabs(r0) + fabs(r1);
  w = (absr > huber) ? (huber / absr) : 1.0;
  const double fxinvz = cam[0] * invz, fyinvz = cam[1] * invz;
  const double nx = -(fxinvz * xinvz), ny = -(fyinvz * yinvz);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    G[c] = fma(fxinvz, Rc[c], nx * Rc[6 + c]);
    G[3 + c] = fma(fyinvz, Rc[3 + c], ny * Rc[6 + c]);
  }
}

// Symmetric 3x3 inverse by diagonally pivoted LDL^T with D pseudo-inverted —
// the behaviour of Eigen's C.ldlt().solve(I) (reference :854): an all-zero
// C_i (never-observed landmark) yields Cinv = 0, not NaN.
// c = {c00 c01 c02 c11 c12 c22}; out in the same order.
__device__ __forceinline__ void ldlt3_inverse(const double c[6], double o[6]) {
  double a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
  // pivot order = selection by |diag| (left-looking: untouched diagonal)
  int s0 = 0;  // 0: none, 1: swap(0,1), 2: swap(0,2)
  {
    double m = fabs(a00);
    if (fabs(a11) > m) {
      m = fabs(a11);
      s0 = 1;
    }
    if (fabs(a22) > m) s0 = 2;
  }
  double t;
  if (s0 == 1) {
    t = a00; a00 = a11; a11 = t;
    t = a02; a02 = a12; a12 = t;
  } else if (s0 == 2) {
    t = a00; a00 = a22; a22 = t;
    t = a01; a01 = a12; a12 = t;
  }
  const bool s1 = fabs(a22) > fabs(a11);
  if (s1) {
    t = a11; a11 = a22; a22 = t;
    t = a01; a01 = a02; a02 = t;
  }
  double b00 = 0, b01 = 0, b02 = 0, b11 = 0, b12 = 0, b22 = 0;
  const double d0 = a00;
  if (fabs(d0) > 0.0) {
    const double l10 = a01 / d0, l20 = a02 / d0;
    const double tmp0 = d0 * l10;
    const double d1 = a11 - l10 * tmp0;
    double l21 = a12 - l20 * tmp0;
    if (fabs(d1) > 0.0) l21 /= d1;
    const double d2 = a22 - (l20 * (d0 * l20) + l21 * (d1 * l21));
    const double tol = 2.2250738585072014e-308;
    const double i0 = (fabs(d0) > tol) ? 1.0 / d0 : 0.0;
    const double i1 = (fabs(d1) > tol) ? 1.0 / d1 : 0.0;
    const double i2 = (fabs(d2) > tol) ? 1.0 / d2 : 0.0;
    // columns of the inverse: solve L D L^T x = e_c
    // e0: z = (1, -l10, -l20 + l21 l10)
    {
      const double z0 = 1.0, z1 = -l10 * z0, z2 = -l20 * z0 - l21 * z1;
      const double w0 = z0 * i0, w1 = z1 * i1, w2 = z2 * i2;
      const double x2 = w2, x1 = w1 - l21 * x2, x0 = w0 - l10 * x1 - l20 * x2;
      b00 = x0;
      (void)x1;
      (void)x2;
    }
    {
      const double z1 = 1.0, z2 = -l21 * z1;
      const double w1 = z1 * i1, w2 = z2 * i2;
      const double x2 = w2, x1 = w1 - l21 * x2, x0 = -l10 * x1 - l20 * x2;
      b01 = x0;
      b11 = x1;
    }
    {
      const double w2 = i2;
      const double x2 = w2, x1 = -l21 * x2, x0 = -l10 * x1 - l20 * x2;
      b02 = x0;
      b12 = x1;
      b22 = x2;
    }
  }
  // undo the symmetric permutations (involutions, reverse order)
  if (s1) {
    t = b11; b11 = b22; b22 = t;
    t = b01; b01 = b02; b02 = t;
  }
  if (s0 == 1) {
    t = b00; b00 = b11; b11 = t;
    t = b02; b02 = b12; b12 = t;
  } else if (s0 == 2) {
    t = b00; b00 = b22; b22 = t;
    t = b01; b01 = b12; b12 = t;
  }
  o[0] = b00; o[1] = b01; o[2] = b02; o[3] = b11; o[4] = b12; o[5] = b22;
}

// The same inverse on its fast path: C_i with a damped diagonal is symmetric
// positive definite for every observed landmark, and LDL^T without pivoting is
// backward stable for such a matrix: three reciprocals (v_rcp_f64 + two Newton
// steps instead of IEEE divisions) and no pivot search / permutation selects — a
// third of the instructions of the pivoted routine, which remains the fallback
// whenever a pivot is not safely positive (below 1e-6 of the largest diagonal entry:
// cond(C_i) > ~1e6): the degenerate cases (never-observed landmark, rank-deficient
// C_i) keep Eigen's pseudo-inverse semantics exactly, and an ill-conditioned C_i — a
// landmark whose depth is barely observable, the ones the LM loop lets run away once
// lambda has fallen — is inverted with the reference's own pivot order (multipliers
// <= 1: no overflow of the inverse where the unpivoted order has |l21| ~ 1e3).
__device__ __forceinline__ double rcp_newton(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.0), r, r);
  r = fma(fma(-d, r, 1.0), r, r);
  return r;
}
__device__ __forceinline__ void spd3_inverse(const double c[6], double o[6]) {
  const double a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
  const double thr = 1e-6 * fmax(a00, fmax(a11, a22));
  const double i0 = rcp_newton(a00);
  const double l10 = a01 * i0, l20 = a02 * i0;
  const double d1 = fma(-l10, a01, a11);
  const double t21 = fma(-l20, a01, a12);
  const double i1 = rcp_newton(d1);
  const double l21 = t21 * i1;
  const double d2 = fma(-l21, t21, fma(-l20, a02, a22));
  const double i2 = rcp_newton(d2);
  if (!(a00 > thr && d1 > thr && d2 > thr) || !(thr > 0.0)) {  // (also NaN / zero matrices)
    ldlt3_inverse(c, o);
    return;
  }
  // inverse = L^-T D^-1 L^-1 with L^-1 = [1 0 0; -l10 1 0; l10 l21 - l20, -l21, 1]
  const double m20 = fma(l10, l21, -l20);
  const double w2 = m20 * i2, v2 = l21 * i2;
  o[5] = i2;                                  // (2,2)
  o[4] = -v2;                                 // (1,2)
  o[2] = w2;                                  // (0,2)
  o[3] = fma(l21, v2, i1);                    // (1,1) = i1 + l21^2 i2
  o[1] = fma(-l10, i1, -(l21 * w2));          // (0,1) = -l10 i1 - l21 m20 i2
  o[0] = fma(m20, w2, fma(l10 * l10, i1, i0));  // (0,0) = i0 + l10^2 i1 + m20^2 i2
}

// se3 exponential of x = (v, w) (reference :1370-1409): exp(x) = [dR, dt] with dR the
// Rodrigues rotation of w and dt = V v.  Shared by the LM pose update and the
// gradient-descent update (k_gd_update), so both move a pose by the same arithmetic.
__device__ __forceinline__ void se3_exp(const double v0, const double v1, const double v2, const double w0,
                                        const double w1, const double w2, double dR[9], double dt[3]) {
  const double theta = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
  const double wx[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
  double wx2[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      wx2[r * 3 + c] = wx[r * 3 + 0] * wx[0 * 3 + c] +
                       wx[r * 3 + 1] * wx[1 * 3 + c] +
                       wx[r * 3 + 2] * wx[2 * 3 + c];
  double ca, cb, va, vb;
  if (theta < 1e-7) {
    ca = 1.0;
    cb = 0.5;
    va = 0.5;
    vb = 0.33333333333333333333333333;
  } else {
    const double st = sin(theta), ct = cos(theta);
    ca = st / theta;
    cb = (1.0 - ct) / (theta * theta);
    va = cb;
    vb = (theta - st) / (theta * theta * theta);
  }
  double V[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double id = (k % 4 == 0) ? 1.0 : 0.0;
    dR[k] = id + ca * wx[k] + cb * wx2[k];
    V[k] = id + va * wx[k] + vb * wx2[k];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
    dt[r] = V[r * 3 + 0] * v0 + V[r * 3 + 1] * v1 + V[r * 3 + 2] * v2;
}

// se3 logarithm, the inverse of se3_exp: x = (v, w) with exp(x) = [R, t].  theta from
// atan2(|vee(R - R^T)| / 2, (tr R - 1) / 2), w = theta / (2 sin theta) vee(R - R^T),
// v = V^-1 t with V^-1 = I - wx / 2 + k wx^2, k = (1 - theta sin theta / (2 (1 - cos theta)))
// / theta^2 (evaluated from theta, not from the trace, which cancels at small angles); below se3_exp's threshold theta < 1e-7 the series w = vee(R - R^T) / 2,
// k = 1 / 12.  Defined for theta < pi (sin theta -> 0 at pi): callers keep the tangent small.
__device__ __forceinline__ void se3_log(const double R[9], const double t[3], double x[6]) {
  const double a0 = R[7] - R[5], a1 = R[2] - R[6], a2 = R[3] - R[1];  // vee(R - R^T)
  const double sn = 0.5 * sqrt(a0 * a0 + a1 * a1 + a2 * a2);
  const double cs = 0.5 * (R[0] + R[4] + R[8] - 1.0);
  const double theta = atan2(sn, cs);
  double f, k;
  if (theta < 1e-7) {
    f = 0.5;
    k = 0.08333333333333333333333333;
  } else {
    const double hf = 0.5 * theta;  // theta sin theta / (2 (1 - cos theta)) = hf cot hf, from theta
    f = theta / (2.0 * sn);
    k = (1.0 - hf * cos(hf) / sin(hf)) / (theta * theta);
  }
  const double w0 = f * a0, w1 = f * a1, w2 = f * a2;
  // wx t = w x t, wx^2 t = w x (w x t)
  const double c0 = w1 * t[2] - w2 * t[1], c1 = w2 * t[0] - w0 * t[2], c2 = w0 * t[1] - w1 * t[0];
  const double e0 = w1 * c2 - w2 * c1, e1 = w2 * c0 - w0 * c2, e2 = w0 * c1 - w1 * c0;
  x[0] = t[0] - 0.5 * c0 + k * e0;
  x[1] = t[1] - 0.5 * c1 + k * e1;
  x[2] = t[2] - 0.5 * c2 + k * e2;
  x[3] = w0;
  x[4] = w1;
  x[5] = w2;
}

// Trust region, convergence and iteration log (reference :928-1007) of ONE problem; one
// thread.  c: the problem's controller, log / log_cap: its iteration rows, n_obs_all: every
// observation of the problem, n_blocks: optimisable poses + optimisable landmarks.
__device__ __forceinline__ void lm_control_step(DevCtrl *c, DevIterRec *log, const int log_cap,
                                                const double n_obs_all, const int n_blocks,
                                                const double current_cost, const double model_est,
                                                const double sum_y, const double sum_x) {
  if (c->done) return;
  const double model = -model_est;
  const double previous_cost = c->prev_cost;
  double rho = (current_cost - previous_cost) * 100.0 / model;
  int status;
  double lambda = c->lambda;
  if (c->gn) {
    // plain Gauss-Newton of the refactored solver (reference
    // core/full_bundle_adjustment_solver_refactor.cpp:976-982)
    status = 0;
    rho = 0.0;
    c->cur ^= 1;
    c->lcur ^= 1;
  } else {
    if (rho > 0.25) {
      status = 0;
      c->cur ^= 1;   // the trial buffer becomes the accepted one ...
      c->lcur ^= 1;  // ... and so does the linearisation made at the trial point
    } else {
      status = 2;   // keep the reserved parameters (reference :943)
    }
    if (rho > 0.5) {
      lambda = fmax(1e-10, lambda * c->dec_ratio);
      status = 1;
    } else if (rho <= 0.25) {
      lambda = fmin(100.0, lambda * c->inc_ratio);
    }
  }
  c->lambda = lambda;
  const double n_obs = n_obs_all;
  const double average_error = current_cost / n_obs;
  const double cost_change = fabs(current_cost - previous_cost);
  const double total_step = sum_y + sum_x;
  const double avg_step = total_step / (double)n_blocks;
  bool conv = (avg_step < c->thr_step) || (cost_change < c->thr_cost);
  if (c->iter >= c->max_iter - 1) conv = false;
  const unsigned long long now = wall_clock64();
  if (c->iter < log_cap) {
    DevIterRec &I = log[c->iter];
    I.cost = current_cost;
    I.cost_change = cost_change;
    I.average_reprojection_error = average_error;
    I.abs_gradient = 0.0;
    I.abs_step = avg_step;
    I.damping_term = lambda;
    I.iter_time_ms = (double)(now - c->t_last) * 1e-5;  // 100 MHz clock
    I.iteration_status = status;
    I.pad_ = 0;
    I.rho = rho;
    I.model_change = c->gn ? 0.0 : model;
    I.trial_cost = current_cost;
    if (status == 2) {  // reference :995-1000
      I.cost = previous_cost;
      I.cost_change = 0.0;
      I.average_reprojection_error = sqrt(previous_cost / n_obs);
    }
  }
  c->t_last = now;
  c->prev_cost = current_cost;  // even when SKIPPED (reference :1005)
  c->iter += 1;
  c->converged = conv ? 1 : 0;
  if (conv || c->iter >= c->max_iter) c->done = 1;
}

}  // namespace ba
#endif  // BA_DEVICE_FN_H_
