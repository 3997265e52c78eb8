// Stand-alone host check of the validation of the robust kernels of the pose-graph optimisation
// (pgraph_robust_validate_host of bundle_adjustment_solver_amd/csrc/ba_pgraph_host.h, the body of
// ba_pgraph_robust_check), meant for the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/pgraph_robust_host_check.cpp -o /tmp/pgraph_robust_host_check && /tmp/pgraph_robust_host_check
// No GPU and no HIP.  Every array is sized exactly, so that an access past an end is the
// sanitizer's to find; the scale array of a call whose kinds are all 0 is a null pointer, so
// that reading it is too.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../bundle_adjustment_solver_amd/csrc/ba_pgraph_host.h"

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                           \
    }                                                                     \
  } while (0)

static int one_case(int64_t F) {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  std::string err;
  std::vector<int32_t> kind((size_t)F);
  std::vector<double> scale((size_t)F);
  for (int64_t f = 0; f < F; ++f) {
    kind[f] = (int32_t)(f % ba::kPgKinds);
    scale[f] = kind[f] ? 0.5 + (double)f : (f % 8 ? nan : -1.0);  // kind 0: never read, whatever it holds
  }
  REQUIRE(ba::pgraph_robust_validate_host(F, kind.data(), scale.data(), &err) == 0);
  REQUIRE(ba::pgraph_robust_validate_host(F, nullptr, nullptr, &err) == 0);
  REQUIRE(ba::pgraph_robust_validate_host(F, nullptr, scale.data(), &err) == 0);
  std::vector<int32_t> zeros((size_t)F, 0);
  REQUIRE(ba::pgraph_robust_validate_host(F, zeros.data(), nullptr, &err) == 0);
  REQUIRE(ba::pgraph_robust_validate_host(-1, kind.data(), scale.data(), &err) == -1);
  // refusals at the first, the last and a middle factor; the message names the factor
  for (int64_t f : {(int64_t)0, F / 2, F - 1}) {
    const std::string at = "(factor " + std::to_string(f) + ")";
    const int32_t k0 = kind[f];
    const double s0 = scale[f];
    for (int32_t bad_kind : {-1, 4, std::numeric_limits<int32_t>::max(), std::numeric_limits<int32_t>::min()}) {
      kind[f] = bad_kind;
      REQUIRE(ba::pgraph_robust_validate_host(F, kind.data(), scale.data(), &err) == -1);
      REQUIRE(err.find("is not one of 0..3") != err.npos && err.find(at) != err.npos);
    }
    for (int32_t k = 1; k < ba::kPgKinds; ++k) {
      kind[f] = k;
      for (double bad_scale : {0.0, -0.0, -1.0, nan, inf, -inf}) {
        scale[f] = bad_scale;
        REQUIRE(ba::pgraph_robust_validate_host(F, kind.data(), scale.data(), &err) == -1);
        REQUIRE(err.find(at) != err.npos);
        REQUIRE(err.find(std::isfinite(bad_scale) ? "scale must be > 0" : "scale is not finite") != err.npos);
      }
      scale[f] = std::numeric_limits<double>::denorm_min();
      REQUIRE(ba::pgraph_robust_validate_host(F, kind.data(), scale.data(), &err) == 0);
      REQUIRE(ba::pgraph_robust_validate_host(F, kind.data(), nullptr, &err) == -1);
      REQUIRE(err.find("null scale array") != err.npos);
    }
    kind[f] = k0;
    scale[f] = s0;
  }
  REQUIRE(ba::pgraph_robust_validate_host(F, kind.data(), scale.data(), &err) == 0);
  return 0;
}

int main() {
  std::string err;
  REQUIRE(ba::pgraph_robust_validate_host(0, nullptr, nullptr, &err) == 0);
  for (int64_t F : {1, 2, 3, 4, 5, 63, 64, 65, 1000})
    if (one_case(F)) return 1;
  std::printf("PGRAPH ROBUST HOST CHECK PASSED\n");
  return 0;
}
