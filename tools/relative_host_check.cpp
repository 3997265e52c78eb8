// Stand-alone host check of the validation, the packing and the shared list builder of the
// relative-pose factors (bundle_adjustment_solver_amd/csrc/ba_rel_host.h), meant for the host
// sanitizers (tests/test_relative_host_check.py runs it so):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/relative_host_check.cpp -o /tmp/relative_host_check && /tmp/relative_host_check
// No GPU and no HIP.  Every array is sized exactly, so that an access past an end is the
// sanitizer's to find.
#include <algorithm>
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

// The shared list builder against a brute-force statement of the lists (a loop over the
// factors per pose and per block): 6 poses, 0 and 3 fixed; 9 factors with one pair twice in
// one direction (0, 2), one pair in both directions (3, 4), two factors to a fixed pose
// (5, 6) and pose 5, which is only ever a k (7, 8).
template <class KeyOf>
static int builder_case(KeyOf key_of) {
  const int n_pose = 6, F = 9, N = 4;
  const std::vector<int32_t> opt_of = {-1, 0, 1, -1, 2, 3};
  const std::vector<int32_t> j = {1, 4, 1, 2, 4, 0, 4, 1, 2}, k = {2, 1, 2, 4, 2, 1, 3, 5, 5};
  REQUIRE((int)opt_of.size() == n_pose && (int)j.size() == F && (int)k.size() == F);
  ba::RelLists l;
  ba::relative_build_lists(F, j.data(), k.data(), N, opt_of.data(), key_of, &l);
  REQUIRE(l.jk.size() == (size_t)4 * F && l.pptr.size() == (size_t)N + 1 && l.pptr[0] == 0);
  for (int f = 0; f < F; ++f)
    REQUIRE(l.jk[4 * f] == j[f] && l.jk[4 * f + 1] == k[f] && l.jk[4 * f + 2] == opt_of[j[f]] &&
            l.jk[4 * f + 3] == opt_of[k[f]]);
  for (int n = 0; n < N; ++n) {
    std::vector<int32_t> want;
    for (int f = 0; f < F; ++f) {
      if (opt_of[j[f]] == n) want.push_back(f << 1);
      if (opt_of[k[f]] == n) want.push_back(f << 1 | 1);
    }
    REQUIRE(l.pptr[n] <= l.pptr[n + 1] && (size_t)l.pptr[n + 1] <= l.plist.size());
    REQUIRE(want == std::vector<int32_t>(l.plist.begin() + l.pptr[n], l.plist.begin() + l.pptr[n + 1]));
  }
  REQUIRE((size_t)l.pptr[N] == l.plist.size() && l.plist.size() == 16);
  REQUIRE(l.pptr[4] - l.pptr[3] == 2 && (l.plist[l.pptr[3]] & 1) && (l.plist[l.pptr[3] + 1] & 1));  // pose 5
  std::vector<int64_t> keys;
  for (int f = 0; f < F; ++f)
    if (opt_of[j[f]] >= 0 && opt_of[k[f]] >= 0) keys.push_back(key_of(opt_of[j[f]], opt_of[k[f]]).first);
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  REQUIRE(keys.size() == 5 && l.bkey == keys && l.bptr.size() == keys.size() + 1 && l.bptr[0] == 0);
  for (size_t b = 0; b < keys.size(); ++b) {
    std::vector<int32_t> want;
    for (int f = 0; f < F; ++f) {
      const int32_t a = opt_of[j[f]], c = opt_of[k[f]];
      if (a < 0 || c < 0) continue;
      REQUIRE(key_of(a, c).first == key_of(c, a).first && key_of(a, c).second != key_of(c, a).second);
      if (key_of(a, c).first == keys[b]) want.push_back(f << 1 | (key_of(a, c).second ? 1 : 0));
    }
    REQUIRE(l.bptr[b] < l.bptr[b + 1] && (size_t)l.bptr[b + 1] <= l.blist.size());
    REQUIRE(want == std::vector<int32_t>(l.blist.begin() + l.bptr[b], l.blist.begin() + l.bptr[b + 1]));
  }
  REQUIRE((size_t)l.bptr[keys.size()] == l.blist.size() && l.blist.size() == 7);
  // no factor at all: empty lists with their leading pointers
  ba::relative_build_lists(0, nullptr, nullptr, N, opt_of.data(), key_of, &l);
  REQUIRE(l.jk.empty() && l.plist.empty() && l.bkey.empty() && l.blist.empty());
  REQUIRE(l.pptr == std::vector<int32_t>((size_t)N + 1, 0) && l.bptr == std::vector<int32_t>(1, 0));
  return 0;
}

int main() {
  for (int n_pose : {3, 4, 7, 64})
    for (int F : {0, 1, 2, 5, 63, 64, 65, 200})
      if (one_case(n_pose, F)) return 1;
  // the planner's convention (upper blocks (lo, hi) numbered row by row, transposed where
  // j > k) and the pose graph's and the batch's (hi * N + lo, transposed where j < k)
  if (builder_case([](int32_t a, int32_t b) {
        return std::pair<int64_t, bool>((int64_t)std::min(a, b) * 4 + std::max(a, b), a > b);
      }))
    return 1;
  if (builder_case([](int32_t a, int32_t b) {
        return std::pair<int64_t, bool>((int64_t)std::max(a, b) * 4 + std::min(a, b), a < b);
      }))
    return 1;
  std::printf("RELATIVE HOST CHECK PASSED\n");
  return 0;
}
