// Stand-alone host check of the Sim(3) factor (bundle_adjustment_solver_amd/csrc/ba_sim3_fn.h,
// compiled here as plain C++) and of the host side of the Sim(3) pose graph (ba_sim3_host.h),
// meant for the host sanitizers:
//   g++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/sim3_host_check.cpp -o /tmp/sim3_host_check && /tmp/sim3_host_check
// No GPU and no HIP.  Every array is sized exactly, so that an access past an end is the
// sanitizer's to find.  The arithmetic is checked against identities that hold for any closed
// form (round trips, the homomorphism of Ad7, a numerical quadrature of W); the comparison with
// expm / logm is tests/test_sim3_ref.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "../bundle_adjustment_solver_amd/csrc/ba_sim3_fn.h"
#include "../bundle_adjustment_solver_amd/csrc/ba_sim3_host.h"

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                           \
    }                                                                     \
  } while (0)

static double max_abs_diff(const double *a, const double *b, int n) {
  double m = 0.0;
  for (int e = 0; e < n; ++e) m = std::fmax(m, std::fabs(a[e] - b[e]));
  return m;
}

// W v by Gauss-Legendre quadrature of integral_0^1 e^(tau sigma) exp(tau hat(omega)) v d tau on
// 8 panels of 5 points (the integrand is entire; the error is far below 1e-13 for |z| <= 3.2)
static void W_quadrature(const double xi[7], double out[3]) {
  static const double gx[5] = {-0.9061798459386640, -0.5384693101056831, 0.0, 0.5384693101056831, 0.9061798459386640};
  static const double gw[5] = {0.2369268850561891, 0.4786286704993665, 0.5688888888888889, 0.4786286704993665,
                               0.2369268850561891};
  out[0] = out[1] = out[2] = 0.0;
  const int panels = 8;
  for (int p = 0; p < panels; ++p)
    for (int i = 0; i < 5; ++i) {
      const double tau = (p + 0.5 * (gx[i] + 1.0)) / panels, w = 0.5 * gw[i] / panels;
      const double rot[7] = {0, 0, 0, tau * xi[3], tau * xi[4], tau * xi[5], 0.0};
      double S[13];
      ba::sim3_exp(rot, S);
      const double f = w * std::exp(tau * xi[6]);
      for (int r = 0; r < 3; ++r) out[r] += f * (S[3 * r] * xi[0] + S[3 * r + 1] * xi[1] + S[3 * r + 2] * xi[2]);
    }
}

static int check_arithmetic() {
  std::mt19937 gen(3);
  std::normal_distribution<double> N(0.0, 1.0);
  const double thetas[] = {0.0, 1e-12, 0.9e-7, 1.1e-7, 1e-4, 1e-2, 0.0499, 0.0501, 0.3, 0.499, 0.501, 1.0, 3.0};
  const double sigmas[] = {0.0, 1e-12, -1e-7, 1e-4, -1e-2, 0.3, -0.3999, 0.4001, 0.4974, 0.4976, -0.6, 0.7, -0.7, 1.5};
  double worst_rt = 0.0, worst_w = 0.0, worst_inv = 0.0, worst_ad = 0.0;
  for (double th : thetas)
    for (double sg : sigmas) {
      double ax[3] = {N(gen), N(gen), N(gen)};
      const double na = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
      const double xi[7] = {N(gen), 0.7 * N(gen), 0.5 * N(gen), th * ax[0] / na, th * ax[1] / na, th * ax[2] / na, sg};
      double S[13], back[7], Wv[3], Si[13], I[13], id[13] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
      ba::sim3_exp(xi, S);
      ba::sim3_log(S, back);
      worst_rt = std::fmax(worst_rt, max_abs_diff(back, xi, 7));
      W_quadrature(xi, Wv);
      worst_w = std::fmax(worst_w, max_abs_diff(Wv, S + 9, 3));
      ba::sim3_inv(S, Si);
      ba::sim3_mul(S, Si, I);
      worst_inv = std::fmax(worst_inv, max_abs_diff(I, id, 13));
      ba::sim3_mul_inv(S, S, I);
      worst_inv = std::fmax(worst_inv, max_abs_diff(I, id, 13));
      // Ad7(A B) = Ad7(A) Ad7(B)
      const double xb[7] = {N(gen), N(gen), N(gen), 0.4 * N(gen), 0.4 * N(gen), 0.4 * N(gen), 0.3 * N(gen)};
      double B[13], AB[13], AdA[49], AdB[49], AdAB[49], prod[49];
      ba::sim3_exp(xb, B);
      ba::sim3_mul(S, B, AB);
      ba::sim3_Ad(S, AdA);
      ba::sim3_Ad(B, AdB);
      ba::sim3_Ad(AB, AdAB);
      for (int r = 0; r < 7; ++r)
        for (int c = 0; c < 7; ++c) {
          double v = 0.0;
          for (int m = 0; m < 7; ++m) v += AdA[7 * r + m] * AdB[7 * m + c];
          prod[7 * r + c] = v;
        }
      double scale = 1.0;
      for (int e = 0; e < 49; ++e) scale = std::fmax(scale, std::fabs(AdAB[e]));
      worst_ad = std::fmax(worst_ad, max_abs_diff(prod, AdAB, 49) / scale);
    }
  std::printf("round trip %.2e, W against quadrature %.2e, inverse %.2e, Ad7 homomorphism %.2e\n", worst_rt, worst_w,
              worst_inv, worst_ad);
  REQUIRE(worst_rt <= 1e-11 && worst_w <= 1e-11 && worst_inv <= 1e-13 && worst_ad <= 1e-13);
  // the element products against the dense matrix product
  double Om[49], Ad[49], r7[7];
  for (int r = 0; r < 7; ++r) {
    r7[r] = N(gen);
    for (int c = 0; c <= r; ++c) Om[7 * r + c] = Om[7 * c + r] = N(gen);
  }
  const double xe[7] = {0.3, -0.2, 0.5, 0.1, 0.4, -0.3, 0.2};
  double E[13], OA[49], Or[7];
  ba::sim3_exp(xe, E);
  ba::sim3_Ad(E, Ad);
  double quad = 0.0;
  for (int q = 0; q < 49; ++q) OA[q] = ba::factor_OA<7>(Om, Ad, q);
  for (int a = 0; a < 7; ++a) Or[a] = ba::factor_Or<7>(Om, r7, a);
  for (int a = 0; a < 7; ++a) quad += r7[a] * Or[a];
  REQUIRE(std::fabs(quad - ba::factor_quad<7>(Om, r7)) <= 1e-12 * std::fabs(quad));
  for (int q = 0; q < 49; ++q) {
    const int a = q / 7, c = q % 7;
    double v = 0.0, vt = 0.0;
    for (int m = 0; m < 7; ++m) {
      v += Ad[7 * m + a] * OA[7 * m + c];
      vt += Ad[7 * m + c] * OA[7 * m + a];
    }
    REQUIRE(std::fabs(ba::factor_Bk<7>(Ad, OA, q) - v) <= 1e-12 * (1.0 + std::fabs(v)));
    REQUIRE(ba::factor_Bk<7>(Ad, OA, q) == ba::factor_Bk<7>(Ad, OA, 7 * c + a));  // symmetric to the bit
    (void)vt;
  }
  for (int a = 0; a < 7; ++a) {
    double v = 0.0;
    for (int m = 0; m < 7; ++m) v += Ad[7 * m + a] * Or[m];
    REQUIRE(ba::factor_gk<7>(Ad, Or, a) == v);
  }
  return 0;
}

static int check_host(int n_pose, int n_fixed, int n_cl) {
  std::vector<uint8_t> fixed((size_t)n_pose, 0);
  for (int p = 0; p < n_fixed; ++p) fixed[(size_t)p] = 1;
  std::vector<int32_t> j, k;
  auto add = [&](int a, int b) {
    if (fixed[a] && fixed[b]) return;
    j.push_back(a);
    k.push_back(b);
  };
  for (int q = 0; q + 1 < n_pose; ++q) add(q + 1, q);
  for (int c = 0; c < n_cl && n_pose > 3; ++c) {
    const int a = (7 * c) % (n_pose - 2), b = a + 2 + (5 * c) % (n_pose - a - 2);
    if (c % 2) add(a, b); else add(b, a);
    if (c == 0) add(a, b);
  }
  const int64_t F = (int64_t)j.size();
  if (F == 0) return 0;
  std::vector<double> S((size_t)n_pose * 13, 0.5), Z((size_t)F * 13, 0.25), Om((size_t)F * 49);
  for (size_t e = 0; e < Om.size(); ++e) Om[e] = (double)(e % 49);
  std::string err;
  REQUIRE(ba::sim3_validate_host(n_pose, S.data(), fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == 0);
  // without the mask every pose is optimisable (with two fixed poses the factor (1, 0) was left
  // out above, and pose 0 may then be a pose that no factor names)
  if (n_fixed < 2)
    REQUIRE(ba::sim3_validate_host(n_pose, S.data(), nullptr, F, j.data(), k.data(), Z.data(), Om.data(), &err) == 0);
  // every refusal of the values, at the last element of its array
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  struct Bad {
    std::vector<double> *v;
    size_t at;
    double x;
    const char *msg;
  } bad[] = {{&S, S.size() - 1, 0.0, "the scale of S_jw must be > 0"}, {&S, S.size() - 1, -1.0, "the scale of S_jw must be > 0"},
             {&S, S.size() - 1, inf, "the scale of S_jw is not finite"}, {&S, S.size() - 2, nan, "S_jw is not finite"},
             {&S, S.size() - 5, nan, "the rotation of S_jw is not finite"}, {&Z, Z.size() - 1, 0.0, "the scale of Z must be > 0"},
             {&Z, Z.size() - 1, nan, "the scale of Z is not finite"}, {&Z, Z.size() - 2, inf, "Z is not finite"},
             {&Z, Z.size() - 13, nan, "the rotation of Z is not finite"}, {&Om, Om.size() - 1, nan, "Omega is not finite"}};
  for (const Bad &b : bad) {
    const double keep = (*b.v)[b.at];
    (*b.v)[b.at] = b.x;
    REQUIRE(ba::sim3_validate_host(n_pose, S.data(), fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1);
    REQUIRE(err.find(b.msg) == 0);
    REQUIRE(ba::sim3_validate_values(n_pose, b.v == &S ? S.data() : nullptr, F, b.v == &Z ? Z.data() : nullptr,
                                     b.v == &Om ? Om.data() : nullptr, &err) == -1);
    (*b.v)[b.at] = keep;
  }
  REQUIRE(ba::sim3_validate_values(n_pose, nullptr, F, nullptr, nullptr, &err) == 0);
  REQUIRE(ba::sim3_validate_host(0, S.data(), nullptr, F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1);
  REQUIRE(ba::sim3_validate_host(n_pose, nullptr, nullptr, F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1);
  REQUIRE(ba::sim3_validate_host(n_pose, S.data(), nullptr, F, j.data(), k.data(), nullptr, Om.data(), &err) == -1);
  REQUIRE(ba::sim3_validate_host(n_pose, S.data(), nullptr, 0, j.data(), k.data(), Z.data(), Om.data(), &err) == -1);
  // the packed values: Z as given, Omega mirrored from its lower triangle
  std::vector<double> val;
  ba::sim3_pack_values(F, Z.data(), Om.data(), &val);
  REQUIRE(val.size() == (size_t)F * ba::kS3Val);
  for (int64_t f = 0; f < F; ++f)
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) {
        const double want = Om[49 * f + (r >= c ? 7 * r + c : 7 * c + r)];
        REQUIRE(val[(size_t)f * ba::kS3Val + 13 + 7 * r + c] == want);
      }
  // the lists and the tile adjacency at 4 and 9 poses per tile
  ba::PgraphLists l;
  ba::pgraph_build_lists(n_pose, fixed.data(), F, j.data(), k.data(), &l);
  REQUIRE(l.N == n_pose - n_fixed);
  REQUIRE(ba::dense_sim3_per_tile(32) == 4 && ba::dense_sim3_per_tile(64) == 9 && ba::dense_poses_per_tile(32) == 5);
  for (int nb : {32, 64}) {
    const int ppt = ba::dense_sim3_per_tile(nb);
    int ncb = 0;
    std::vector<uint8_t> adj;
    ba::sim3_tile_adjacency(l, nb, &ncb, &adj);
    REQUIRE(ncb == std::max(1, (l.N + ppt - 1) / ppt) && adj.size() == (size_t)ncb * ncb);
    REQUIRE(7 * ppt <= nb);
    for (int a = 0; a < ncb; ++a) {
      REQUIRE(adj[(size_t)a * ncb + a] == 0);
      for (int b = 0; b < ncb; ++b) REQUIRE(adj[(size_t)a * ncb + b] == adj[(size_t)b * ncb + a]);
    }
    for (size_t b = 0; b + 1 < l.blk.size(); b += 2) {
      const int I = l.blk[b] / ppt, J = l.blk[b + 1] / ppt;
      REQUIRE(I < ncb && J < ncb && (I == J || adj[(size_t)I * ncb + J] == 1));
    }
  }
  return 0;
}

int main() {
  if (check_arithmetic()) return 1;
  for (int n_pose : {2, 5, 6, 10, 11, 37, 60})
    for (int n_fixed : {0, 1, 2})
      for (int n_cl : {0, 1, 4})
        if (n_fixed < n_pose && check_host(n_pose, n_fixed, n_cl)) return 1;
  std::printf("SIM3 HOST CHECK PASSED\n");
  return 0;
}
