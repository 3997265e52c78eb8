// Stand-alone host check (its own main, no HIP, no GPU) of the plain-C++ pieces behind the robust
// kernels, the covariance blocks and the gate of the Sim(3) graph:
//   pg_rho (csrc/ba_robust_fn.h): rho and w of every kind against long-double restatements of the
//       table of include/ba_hip.h, w against a central difference of rho, w(0) = 1;
//   chol_host at width 7 (csrc/ba_pgraph_host.h): accepts J^T J of random 9x7 J and reproduces it from
//       a long-double Cholesky to 1e-12, refuses a zero, an indefinite, a rank-6 and a NaN matrix,
//       reads the lower triangle only;
//   sim3_cov_validate_host: one refusal of each family and an accepted call.
// Build and run, e.g. under the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Ibundle_adjustment_solver_amd/csrc \
//       tools/sim3_cov_host_check.cpp -o /tmp/sim3_cov_host_check && /tmp/sim3_cov_host_check
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "ba_robust_fn.h"
#include "ba_sim3_host.h"

static int fails = 0;
#define EXPECT(cond)                                        \
  do {                                                      \
    if (!(cond)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++fails;                                              \
    }                                                       \
  } while (0)

static long double rho_ld(int kind, long double c, long double s, long double *w) {
  const long double c2 = c * c;
  if (kind == 1 && s > c2) {
    *w = c / sqrtl(s);
    return 2.0L * c * sqrtl(s) - c2;
  }
  if (kind == 2) {
    *w = 1.0L / (1.0L + s / c2);
    return c2 * log1pl(s / c2);
  }
  if (kind == 3) {
    *w = (c2 / (c2 + s)) * (c2 / (c2 + s));
    return c2 * s / (c2 + s);
  }
  *w = 1.0L;
  return s;
}

int main() {
  // ---- rho and w
  double worst = 0.0;
  for (int kind = 0; kind < 4; ++kind)
    for (double c : {1e-3, 1.0, 30.0, 1e4})
      for (double u : {0.0, 1e-12, 0.5, 0.999999, 1.000001, 2.0, 1e3, 1e12}) {
        const double s = u * c * c;
        double w = 0.0;
        const double r = ba::pg_rho(kind, c, s, &w);
        long double wl = 0.0L;
        const long double rl = rho_ld(kind, c, s, &wl);
        worst = std::fmax(worst, std::fabs((double)((r - rl) / (rl == 0.0L ? 1.0L : rl))));
        worst = std::fmax(worst, std::fabs((double)((w - wl) / wl)));
        if (u == 0.0) EXPECT(w == 1.0 && r == 0.0);
        if (u >= 0.5 && u <= 1e3 && !(kind == 1 && std::fabs(u - 1.0) < 1e-3)) {  // w = d rho / d s
          double wa, wb;
          const double h = 1e-6 * s;
          const double d = (ba::pg_rho(kind, c, s + h, &wa) - ba::pg_rho(kind, c, s - h, &wb)) / (2.0 * h);
          EXPECT(std::fabs(d - w) <= 1e-6 * std::fmax(1.0, std::fabs(w)));
        }
      }
  std::printf("rho and w against long double: %.2e relative\n", worst);
  EXPECT(worst <= 1e-14);
  // ---- chol_host at width 7
  std::mt19937 gen(7);
  std::normal_distribution<double> N(0.0, 1.0);
  double O[49], worst_c = 0.0;
  for (int trial = 0; trial < 50; ++trial) {
    double J[63];
    for (double &v : J) v = N(gen) * (trial % 5 == 0 ? 1e3 : 1.0);
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) {
        double a = 0.0;
        for (int m = 0; m < 9; ++m) a += J[7 * m + r] * J[7 * m + c];
        O[7 * r + c] = r >= c ? a : 1e300;  // the upper triangle is never read
      }
    EXPECT(ba::chol_host(O, 7));
    long double L[49] = {0.0L};
    bool ok = true;
    for (int c = 0; c < 7 && ok; ++c) {
      long double d = O[7 * c + c];
      for (int m = 0; m < c; ++m) d -= L[7 * c + m] * L[7 * c + m];
      ok = d > 0.0L;
      L[7 * c + c] = sqrtl(d);
      for (int r = c + 1; r < 7; ++r) {
        long double v = O[7 * r + c];
        for (int m = 0; m < c; ++m) v -= L[7 * r + m] * L[7 * c + m];
        L[7 * r + c] = v / L[7 * c + c];
      }
    }
    EXPECT(ok);
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c <= r; ++c) {
        long double a = 0.0L;
        for (int m = 0; m <= c; ++m) a += L[7 * r + m] * L[7 * c + m];
        worst_c = std::fmax(worst_c, std::fabs((double)((a - O[7 * r + c]) / O[7 * r + r])));
      }
  }
  std::printf("L L^T against Omega: %.2e relative\n", worst_c);
  EXPECT(worst_c <= 1e-12);
  double Zr[49] = {0.0};
  EXPECT(!ba::chol_host(Zr, 7));
  for (int r = 0; r < 7; ++r) Zr[8 * r] = 1.0;
  EXPECT(ba::chol_host(Zr, 7));
  Zr[8 * 3] = -1.0;
  EXPECT(!ba::chol_host(Zr, 7));
  Zr[8 * 3] = 1.0;
  Zr[8 * 6] = 0.0;  // rank 6
  EXPECT(!ba::chol_host(Zr, 7));
  Zr[8 * 6] = std::nan("");
  EXPECT(!ba::chol_host(Zr, 7));
  // ---- the validation
  const uint8_t fixed[4] = {1, 0, 0, 0};
  const int32_t sel[2] = {1, 3}, bad_sel[2] = {1, 0}, pj[2] = {1, 0}, pk[2] = {2, 3}, same[2] = {2, 0};
  double out[98] = {0.0}, Z[26] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, Om[98] = {0.0};
  for (int c = 0; c < 2; ++c)
    for (int r = 0; r < 7; ++r) Om[49 * c + 8 * r] = 2.0;
  std::string err;
  EXPECT(ba::sim3_cov_validate_host(4, fixed, 2, sel, out, 2, pj, pk, out, 2, pj, pk, Z, Om, out, &err) == 0);
  EXPECT(ba::sim3_cov_validate_host(4, fixed, 2, bad_sel, out, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                    nullptr, nullptr, &err) != 0 &&
         err == "ba_sim3_covariance: pose_sel[1] = 0 is a fixed pose");
  EXPECT(ba::sim3_cov_validate_host(4, fixed, 0, nullptr, nullptr, 2, pj, same, out, 0, nullptr, nullptr, nullptr, nullptr,
                                    nullptr, &err) != 0 &&
         err == "ba_sim3_covariance: j == k: a factor needs two distinct poses (pair 1)");
  Z[25] = 0.0;
  EXPECT(ba::sim3_cov_validate_host(4, fixed, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 2, pj, pk, Z, Om, out,
                                    &err) != 0 &&
         err == "ba_sim3_gate: the scale of Z must be > 0 (candidate 1)");
  Z[25] = 1.0;
  Z[4] = std::nan("");
  EXPECT(ba::sim3_cov_validate_host(4, fixed, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 2, pj, pk, Z, Om, out,
                                    &err) != 0 &&
         err == "ba_sim3_gate: the rotation of Z is not finite (candidate 0)");
  Z[4] = 1.0;
  Om[49 + 8 * 2] = -2.0;
  EXPECT(ba::sim3_cov_validate_host(4, fixed, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 2, pj, pk, Z, Om, out,
                                    &err) != 0 &&
         err == "ba_sim3_gate: Omega is not positive definite (candidate 1)");
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("SIM3 COV HOST CHECK PASSED\n");
  return 0;
}
