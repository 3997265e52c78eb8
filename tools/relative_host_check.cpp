// Stand-alone host check of the validation and packing of the handle path's relative-pose
// factors (bundle_adjustment_solver_amd/csrc/ba_rel_host.h), meant for the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/relative_host_check.cpp -o /tmp/relative_host_check && /tmp/relative_host_check
// No GPU and no HIP.  Every array is sized exactly, so that an access past an end is the
// sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../bundle_adjustment_solver_amd/csrc/ba_rel_host.h"

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                           \
    }                                                                     \
  } while (0)

static int one_case(int n_pose, int F) {
  std::vector<uint8_t> fixed((size_t)n_pose, 0);
  fixed[0] = 1;
  if (n_pose > 3) fixed[1] = 1;
  std::vector<int32_t> j((size_t)F), k((size_t)F);
  std::vector<double> Z((size_t)F * 12), Om((size_t)F * 36);
  for (int f = 0; f < F; ++f) {
    j[f] = 2 + f % (n_pose - 2);
    k[f] = (j[f] + 1 + f % (n_pose - 1)) % n_pose;
    if (k[f] == j[f]) k[f] = 0;
    for (int e = 0; e < 12; ++e) Z[12 * (size_t)f + e] = f + 0.01 * e;
    for (int e = 0; e < 36; ++e) Om[36 * (size_t)f + e] = 100.0 * f + e;  // not symmetric: the lower triangle counts
  }
  const int all = ba::kRelPairs | ba::kRelValues;
  std::string err;
  REQUIRE(ba::relative_validate_host(all, n_pose, fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == 0);
  REQUIRE(ba::relative_validate_host(all, n_pose, nullptr, F, j.data(), k.data(), Z.data(), Om.data(), &err) == 0);
  REQUIRE(ba::relative_validate_host(ba::kRelPairs, n_pose, fixed.data(), F, j.data(), k.data(), nullptr, nullptr, &err) == 0);
  REQUIRE(ba::relative_validate_host(ba::kRelValues, n_pose, nullptr, F, nullptr, nullptr, Z.data(), Om.data(), &err) == 0);
  std::vector<double> val;
  ba::relative_pack_values(F, Z.data(), Om.data(), &val);
  REQUIRE(val.size() == (size_t)F * ba::kRelVal);
  for (int f = 0; f < F; ++f) {
    const double *v = val.data() + (size_t)f * ba::kRelVal;
    for (int e = 0; e < 12; ++e) REQUIRE(v[e] == Z[12 * (size_t)f + e]);
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        REQUIRE(v[12 + r * 6 + c] == v[12 + c * 6 + r]);
        if (r >= c) REQUIRE(v[12 + r * 6 + c] == Om[36 * (size_t)f + r * 6 + c]);
      }
  }
  if (F == 0) return 0;
  // refusals: the message names the factor; the last factor is the one at the arrays' ends
  const int l = F - 1;
  const std::string at = "(factor " + std::to_string(l) + ")";
  const int32_t jl = j[l], kl = k[l];
  j[l] = n_pose;
  REQUIRE(ba::relative_validate_host(all, n_pose, fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1 &&
          err.find("pose j") != err.npos && err.find(at) != err.npos);
  j[l] = -1;
  REQUIRE(ba::relative_validate_host(all, n_pose, fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1);
  j[l] = jl;
  k[l] = n_pose + 5;
  REQUIRE(ba::relative_validate_host(all, n_pose, fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1 &&
          err.find("pose k") != err.npos && err.find(at) != err.npos);
  k[l] = jl;
  REQUIRE(ba::relative_validate_host(all, n_pose, fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1 &&
          err.find("j == k") != err.npos);
  if (n_pose > 3) {
    j[l] = 0;
    k[l] = 1;
    REQUIRE(ba::relative_validate_host(all, n_pose, fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1 &&
            err.find("both poses are fixed") != err.npos && err.find(at) != err.npos);
    REQUIRE(ba::relative_validate_host(all, n_pose, nullptr, F, j.data(), k.data(), Z.data(), Om.data(), &err) == 0);
  }
  j[l] = jl;
  k[l] = kl;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  Z[12 * (size_t)l + 11] = nan;
  REQUIRE(ba::relative_validate_host(all, n_pose, fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1 &&
          err.find("Z is not finite") != err.npos && err.find(at) != err.npos);
  REQUIRE(ba::relative_validate_host(ba::kRelPairs, n_pose, fixed.data(), F, j.data(), k.data(), nullptr, nullptr, &err) == 0);
  Z[12 * (size_t)l + 11] = 0.0;
  Om[36 * (size_t)l + 35] = inf;
  REQUIRE(ba::relative_validate_host(ba::kRelValues, n_pose, nullptr, F, nullptr, nullptr, Z.data(), Om.data(), &err) == -1 &&
          err.find("Omega is not finite") != err.npos && err.find(at) != err.npos);
  Om[36 * (size_t)l + 35] = 1.0;
  REQUIRE(ba::relative_validate_host(all, n_pose, fixed.data(), F, nullptr, k.data(), Z.data(), Om.data(), &err) == -1);
  REQUIRE(ba::relative_validate_host(all, n_pose, fixed.data(), F, j.data(), k.data(), Z.data(), nullptr, &err) == -1);
  REQUIRE(ba::relative_validate_host(all, n_pose, fixed.data(), -1, j.data(), k.data(), Z.data(), Om.data(), &err) == -1);
  REQUIRE(ba::relative_validate_host(all, 0, nullptr, F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1);
  return 0;
}

int main() {
  for (int n_pose : {3, 4, 7, 64})
    for (int F : {0, 1, 2, 5, 63, 64, 65, 200})
      if (one_case(n_pose, F)) return 1;
  std::printf("RELATIVE HOST CHECK PASSED\n");
  return 0;
}
