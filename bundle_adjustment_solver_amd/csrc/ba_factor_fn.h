// ba_factor_fn.h — the five element functions of a relative factor at tangent width W, once: W = 6
// for the SE(3) factor (rel_* of ba_rel_fn.h forward here), W = 7 for the Sim(3) factor (sim3_* of
// ba_sim3_fn.h).  Om is the factor's W x W information matrix mirrored by the host, Ad its W x W
// adjoint, both row-major.  __host__ __device__, so that tools/sim3_host_check.cpp (a plain C++
// compiler) runs this text too; forced inline, and the library builds with -ffp-contract=off, so
// that one expression gives the same bits in every caller.
#ifndef BA_FACTOR_FN_H_
#define BA_FACTOR_FN_H_

#if defined(__HIPCC__)
#define BA_FACTOR_FN __host__ __device__ __forceinline__
#else
#define BA_FACTOR_FN inline
#endif

namespace ba {

// r^T Omega r
template <int W>
BA_FACTOR_FN double factor_quad(const double *Om, const double *r) {
  double q = 0.0;
#pragma unroll
  for (int a = 0; a < W; ++a) {
    double row = 0.0;
#pragma unroll
    for (int c = 0; c < W; ++c) row += Om[a * W + c] * r[c];
    q += r[a] * row;
  }
  return q;
}

// The per-element threads take element e < W W + W of a pair {W x W block, W-vector}: q = e < W W
// of the block, else a = e - W W of the vector.  Each caller keeps that branch, with its stores in
// it.  The products are dense: the zeros of an adjoint are added as zeros, so that a sparse form
// would have to give these bits.
// element q of OA = Omega Ad and element a of Or = Omega r
template <int W>
BA_FACTOR_FN double factor_OA(const double *Om, const double *Ad, const int q) {
  const int a = q / W, c = q - W * a;
  double acc = 0.0;
  for (int m = 0; m < W; ++m) acc += Om[a * W + m] * Ad[m * W + c];
  return acc;
}
template <int W>
BA_FACTOR_FN double factor_Or(const double *Om, const double *r, const int a) {
  double acc = 0.0;
  for (int m = 0; m < W; ++m) acc += Om[a * W + m] * r[m];
  return acc;
}

// element q of Bk = Ad^T OA, from the expression of its lower-triangle twin, so that Bk is
// symmetric to the bit, and element a of gk = Ad^T Or
template <int W>
BA_FACTOR_FN double factor_Bk(const double *Ad, const double *OA, const int q) {
  const int r0 = q / W, c0 = q - W * r0;
  const int a = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
  double acc = 0.0;
  for (int m = 0; m < W; ++m) acc += Ad[m * W + a] * OA[m * W + c];
  return acc;
}
template <int W>
BA_FACTOR_FN double factor_gk(const double *Ad, const double *Or, const int a) {
  double acc = 0.0;
  for (int m = 0; m < W; ++m) acc += Ad[m * W + a] * Or[m];
  return acc;
}

}  // namespace ba
#endif  // BA_FACTOR_FN_H_
