// ba_robust_fn.h — the robust kernels of a pose-graph factor, once (include/ba_hip.h, the table
// of ba_pgraph_set_robust): rho(s) and w = rho'(s) of s = r^T Omega r for
// kind 0 none, 1 Huber, 2 Cauchy, 3 Geman-McClure with scale c.  The robust instantiations of
// ba_pgraph.hip and ba_sim3.hip call it, and tools/sim3_cov_host_check.cpp (a plain C++ compiler)
// runs the same text on the host.  Forced inline.
#ifndef BA_ROBUST_FN_H_
#define BA_ROBUST_FN_H_

#include <cmath>

#if defined(__HIPCC__)
#define BA_ROBUST_FN __host__ __device__ __forceinline__
#else
#define BA_ROBUST_FN inline
#endif

namespace ba {

// rho(s) and w = rho'(s) of one factor; s = 0 gives w = 1 for every kind
BA_ROBUST_FN double pg_rho(int kind, double c, double s, double *w) {
  const double c2 = c * c;
  if (kind == 1) {
    if (s <= c2) {
      *w = 1.0;
      return s;
    }
    const double rs = sqrt(s);
    *w = c / rs;
    return 2.0 * c * rs - c2;
  }
  if (kind == 2) {
    const double u = s / c2;
    *w = 1.0 / (1.0 + u);
    return c2 * log1p(u);
  }
  if (kind == 3) {
    const double t = c2 / (c2 + s);
    *w = t * t;
    return t * s;
  }
  *w = 1.0;
  return s;
}

}  // namespace ba
#endif  // BA_ROBUST_FN_H_
