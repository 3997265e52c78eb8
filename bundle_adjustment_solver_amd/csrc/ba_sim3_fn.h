// ba_sim3_fn.h — the Sim(3) factor, once (the definition is the comment of
// ba_sim3_create in include/ba_hip.h).  A similarity S = (R, t, s) is 13 doubles {R row-major,
// t, s} and maps x -> s R x + t; the tangent is xi = [v; omega; sigma].  Factor f between the
// poses j and k: E = S_j S_k^-1, r = sim3_log(E Z^-1), first-order Jacobians dr/dxi_j = I and
// dr/dxi_k = -Ad7(E), so that with Omega mirrored by the host
//   H_jj += Omega           g_j += -Omega r          H_jk += -Omega Ad7
//   H_kk += Ad7^T Omega Ad7 g_k += Ad7^T Omega r
// The functions are __host__ __device__: the kernels of ba_sim3.hip, the host-only ABI entries
// ba_sim3_exp / ba_sim3_log / ba_sim3_adjoint and tools/sim3_host_check.cpp (a plain C++
// compiler) run this one text.  Every function is forced inline and the library builds with
// -ffp-contract=off, so that one expression gives the same bits in every kernel.
#ifndef BA_SIM3_FN_H_
#define BA_SIM3_FN_H_

#include <cmath>
#include <cstddef>

#include "ba_factor_fn.h"

#if defined(__HIPCC__)
#define BA_S3_FN __host__ __device__ __forceinline__
#else
#define BA_S3_FN inline
#endif

namespace ba {

// W = integral_0^1 e^(tau sigma) exp(tau hat(omega)) d tau = C I + A hat(omega) + B hat(omega)^2.
// With z = sigma + i theta and phi(z) = (e^z - 1) / z = integral_0^1 e^(tau z) d tau:
//   C = phi(sigma),  A = Im phi(z) / theta,  B = (phi(sigma) - Re phi(z)) / theta^2.
// Three evaluations, each used where it keeps 1e-13 or better (th2 = theta^2):
//   |z|^2 < kS3SeriesZ2   the power series of phi: with p_n = Re z^n, q_n = Im z^n / theta and
//                         d_n = (sigma^n - Re z^n) / theta^2 the sums of q_n, d_n and sigma^n over
//                         (n + 1)! have no cancellation and no division by theta or sigma
//                         (q_{n+1} = sigma q_n + p_n, d_{n+1} = sigma d_n + q_n,
//                         p_{n+1} = sigma p_n - theta^2 q_n); 16 terms: 0.5^16 / 17! < 1e-19
//   theta >= kS3SmallTheta the closed form of phi(z) (rounding eps e^sigma / theta^2)
//   otherwise             (|sigma| >= 0.49) the series in theta with the moments
//                         M_k = integral tau^k e^(tau sigma) = (e^sigma - k M_{k-1}) / sigma; the
//                         truncation is theta^8 / 9! < 1e-16
constexpr double kS3SeriesZ2 = 0.25;
constexpr double kS3SmallTheta = 0.05;
BA_S3_FN void sim3_W_coef(const double sigma, const double th2, double *A, double *B, double *C) {
  if (sigma * sigma + th2 < kS3SeriesZ2) {
    double p = 1.0, q = 0.0, d = 0.0, sn = 1.0;  // n = 0
    double a = 0.0, b = 0.0, c = 1.0, inv = 1.0;  // inv = 1 / (n + 1)!
#pragma unroll
    for (int n = 1; n <= 16; ++n) {
      const double pn = sigma * p - th2 * q, qn = sigma * q + p, dn = sigma * d + q;
      p = pn;
      q = qn;
      d = dn;
      sn *= sigma;
      inv /= (double)(n + 1);
      a += q * inv;
      b += d * inv;
      c += sn * inv;
    }
    *A = a;
    *B = b;
    *C = c;
    return;
  }
  const double s = exp(sigma);
  const double c0 = sigma == 0.0 ? 1.0 : expm1(sigma) / sigma;
  *C = c0;
  if (th2 >= kS3SmallTheta * kS3SmallTheta) {
    const double theta = sqrt(th2), st = sin(theta), ct = cos(theta);
    const double z2 = sigma * sigma + th2;
    const double er = s * ct - 1.0, ei = s * st;  // e^z - 1
    *A = (ei * sigma - er * theta) / (z2 * theta);
    *B = (c0 - (er * sigma + ei * theta) / z2) / th2;
    return;
  }
  double M[9];
  M[0] = c0;
#pragma unroll
  for (int k = 1; k <= 8; ++k) M[k] = (s - (double)k * M[k - 1]) / sigma;
  const double t4 = th2 * th2, t6 = t4 * th2;
  *A = M[1] - th2 * M[3] / 6.0 + t4 * M[5] / 120.0 - t6 * M[7] / 5040.0;
  *B = 0.5 * M[2] - th2 * M[4] / 24.0 + t4 * M[6] / 720.0 - t6 * M[8] / 40320.0;
}

// sim3_exp(xi) = (exp(hat(omega)), W v, e^sigma).  The rotation is se3_exp's Rodrigues form with
// its threshold.
BA_S3_FN void sim3_exp(const double xi[7], double S[13]) {
  const double w0 = xi[3], w1 = xi[4], w2 = xi[5], sigma = xi[6];
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2, theta = sqrt(th2);
  const double wx[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
  double wx2[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      wx2[r * 3 + c] = wx[r * 3 + 0] * wx[0 * 3 + c] + wx[r * 3 + 1] * wx[1 * 3 + c] + wx[r * 3 + 2] * wx[2 * 3 + c];
  double ca, cb;
  if (theta < 1e-7) {
    ca = 1.0;
    cb = 0.5;
  } else {
    const double hs = sin(0.5 * theta);
    ca = sin(theta) / theta;
    cb = 2.0 * hs * hs / th2;  // (1 - cos theta) / theta^2 without the cancellation
  }
  double A, B, C;
  sim3_W_coef(sigma, th2, &A, &B, &C);
  double W[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double id = (k % 4 == 0) ? 1.0 : 0.0;
    S[k] = id + ca * wx[k] + cb * wx2[k];
    W[k] = C * id + A * wx[k] + B * wx2[k];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) S[9 + r] = W[r * 3 + 0] * xi[0] + W[r * 3 + 1] * xi[1] + W[r * 3 + 2] * xi[2];
  S[12] = exp(sigma);
}

// sim3_log, the inverse of sim3_exp for a rotation angle below pi: sigma = log s, omega as
// se3_log takes it from R, v = W^-1 t.  From hat(omega)^3 = -theta^2 hat(omega):
//   W^-1 = (1 / C) I - (A / det) hat(omega) + ((A^2 - B D) / (C det)) hat(omega)^2,
//   D = C - theta^2 B,  det = D^2 + theta^2 A^2,
// with the A, B, C of sim3_W_coef, so the inverse has no thresholds of its own.
BA_S3_FN void sim3_log(const double S[13], double xi[7]) {
  const double a0 = S[7] - S[5], a1 = S[2] - S[6], a2 = S[3] - S[1];  // vee(R - R^T)
  const double sn = 0.5 * sqrt(a0 * a0 + a1 * a1 + a2 * a2);
  const double cs = 0.5 * (S[0] + S[4] + S[8] - 1.0);
  const double theta = atan2(sn, cs);
  const double f = theta < 1e-7 ? 0.5 : theta / (2.0 * sn);
  const double w0 = f * a0, w1 = f * a1, w2 = f * a2;
  const double sigma = log(S[12]);
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  double A, B, C;
  sim3_W_coef(sigma, th2, &A, &B, &C);
  const double D = C - th2 * B, det = D * D + th2 * A * A;
  const double al = 1.0 / C, be = A / det, ga = (A * A - B * D) / (C * det);
  const double *t = S + 9;
  const double c0 = w1 * t[2] - w2 * t[1], c1 = w2 * t[0] - w0 * t[2], c2 = w0 * t[1] - w1 * t[0];
  const double e0 = w1 * c2 - w2 * c1, e1 = w2 * c0 - w0 * c2, e2 = w0 * c1 - w1 * c0;
  xi[0] = al * t[0] - be * c0 + ga * e0;
  xi[1] = al * t[1] - be * c1 + ga * e1;
  xi[2] = al * t[2] - be * c2 + ga * e2;
  xi[3] = w0;
  xi[4] = w1;
  xi[5] = w2;
  xi[6] = sigma;
}

// out = a b: (R_a R_b, s_a R_a t_b + t_a, s_a s_b).  out may not alias a or b.
BA_S3_FN void sim3_mul(const double *a, const double *b, double *out) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      out[r * 3 + c] = a[r * 3 + 0] * b[0 * 3 + c] + a[r * 3 + 1] * b[1 * 3 + c] + a[r * 3 + 2] * b[2 * 3 + c];
    out[9 + r] = a[12] * (a[r * 3 + 0] * b[9] + a[r * 3 + 1] * b[10] + a[r * 3 + 2] * b[11]) + a[9 + r];
  }
  out[12] = a[12] * b[12];
}

// out = a b^-1: (R_a R_b^T, t_a - (s_a / s_b) R t_b, s_a / s_b).  out may not alias a or b.
BA_S3_FN void sim3_mul_inv(const double *a, const double *b, double *out) {
  const double s = a[12] / b[12];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      out[r * 3 + c] = a[r * 3 + 0] * b[c * 3 + 0] + a[r * 3 + 1] * b[c * 3 + 1] + a[r * 3 + 2] * b[c * 3 + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    out[9 + r] = a[9 + r] - s * (out[r * 3 + 0] * b[9] + out[r * 3 + 1] * b[10] + out[r * 3 + 2] * b[11]);
  out[12] = s;
}

// out = a^-1: (R^T, -R^T t / s, 1 / s).  out may not alias a.
BA_S3_FN void sim3_inv(const double *a, double *out) {
  const double is = 1.0 / a[12];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[r * 3 + c] = a[c * 3 + r];
    out[9 + r] = -is * (a[0 * 3 + r] * a[9] + a[1 * 3 + r] * a[10] + a[2 * 3 + r] * a[11]);
  }
  out[12] = is;
}

// E = S_j S_k^-1 of a factor at the poses P (13 per pose), and its residual r = sim3_log(E Z^-1)
BA_S3_FN void sim3_E(const int j, const int k, const double *P, double E[13]) {
  sim3_mul_inv(P + (size_t)j * 13, P + (size_t)k * 13, E);
}
BA_S3_FN void sim3_res(const double E[13], const double *Z, double r[7]) {
  double D[13];
  sim3_mul_inv(E, Z, D);
  sim3_log(D, r);
}

// Ad7(E) = [[s R, hat(t) R, -t], [0, R, 0], [0, 0, 1]] as 49 doubles, row-major (an LDS row)
BA_S3_FN void sim3_Ad(const double E[13], double *Ad) {
  const double *t = E + 9, s = E[12];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    Ad[0 * 7 + 3 + c] = t[1] * E[6 + c] - t[2] * E[3 + c];
    Ad[1 * 7 + 3 + c] = t[2] * E[0 + c] - t[0] * E[6 + c];
    Ad[2 * 7 + 3 + c] = t[0] * E[3 + c] - t[1] * E[0 + c];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      Ad[a * 7 + c] = s * E[a * 3 + c];
      Ad[(3 + a) * 7 + 3 + c] = E[a * 3 + c];
      Ad[(3 + a) * 7 + c] = 0.0;
    }
    Ad[c * 7 + 6] = -t[c];
    Ad[(3 + c) * 7 + 6] = 0.0;
    Ad[6 * 7 + c] = 0.0;
    Ad[6 * 7 + 3 + c] = 0.0;
  }
  Ad[48] = 1.0;
}

// (r^T Omega r and the elements of Omega Ad7, Omega r, Ad7^T Omega Ad7, Ad7^T Omega r that the
// per-element threads take are factor_quad / ... / factor_gk of ba_factor_fn.h at width 7)

}  // namespace ba
#endif  // BA_SIM3_FN_H_
