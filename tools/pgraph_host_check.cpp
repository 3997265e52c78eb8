// Stand-alone host check of the validation, the factor lists and the tile adjacency of the
// pose-graph optimisation (bundle_adjustment_solver_amd/csrc/ba_pgraph_host.h), meant for the
// host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/pgraph_host_check.cpp -o /tmp/pgraph_host_check && /tmp/pgraph_host_check
// No GPU and no HIP.  Every array is sized exactly, so that an access past an end is the
// sanitizer's to find.
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

// a chain (q + 1, q) plus n_cl closures in alternating orientation, the first one named twice
static int one_case(int n_pose, int n_fixed, int n_cl) {
  std::vector<uint8_t> fixed((size_t)n_pose, 0);
  for (int p = 0; p < n_fixed; ++p) fixed[(size_t)p * (n_pose - 1) / (n_fixed > 1 ? n_fixed - 1 : 1)] = 1;
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
  std::vector<double> T((size_t)n_pose * 12, 0.5), Z((size_t)F * 12, 0.25), Om((size_t)F * 36, 2.0);
  std::string err;
  int rc = ba::pgraph_validate_host(n_pose, T.data(), fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err);
  // a fixed pose in the middle of the chain may leave a neighbour without a factor only if
  // both its neighbours are fixed, which this construction never does
  REQUIRE(rc == 0);
  REQUIRE(ba::pgraph_validate_host(n_pose, T.data(), nullptr, F, j.data(), k.data(), Z.data(), Om.data(), &err) == 0);
  ba::PgraphLists l;
  ba::pgraph_build_lists(n_pose, fixed.data(), F, j.data(), k.data(), &l);
  REQUIRE(l.N == n_pose - n_fixed && (int)l.opt_pose.size() == l.N && (int)l.pptr.size() == l.N + 1);
  REQUIRE(l.jk.size() == (size_t)F * 4 && l.bptr.size() == l.blk.size() / 2 + 1);
  // every factor appears once per optimisable end, in input order per pose
  size_t ends = 0;
  for (int64_t f = 0; f < F; ++f) {
    REQUIRE(l.jk[4 * f] == j[f] && l.jk[4 * f + 1] == k[f]);
    REQUIRE(l.jk[4 * f + 2] == l.opt_of_pose[j[f]] && l.jk[4 * f + 3] == l.opt_of_pose[k[f]]);
    ends += (l.jk[4 * f + 2] >= 0) + (l.jk[4 * f + 3] >= 0);
  }
  REQUIRE(l.plist.size() == ends && (size_t)l.pptr[l.N] == ends);
  for (int n = 0; n < l.N; ++n) {
    REQUIRE(l.pptr[n] < l.pptr[n + 1]);  // validated: every optimisable pose is named
    for (int q = l.pptr[n]; q < l.pptr[n + 1]; ++q) {
      const int w = l.plist[q], f = w >> 1;
      REQUIRE(f >= 0 && f < F && l.jk[4 * f + 2 + (w & 1)] == n);
      if (q > l.pptr[n]) REQUIRE((l.plist[q - 1] >> 1) <= f);
    }
  }
  size_t coupled = 0;
  for (int64_t f = 0; f < F; ++f) coupled += l.jk[4 * f + 2] >= 0 && l.jk[4 * f + 3] >= 0;
  REQUIRE(l.blist.size() == coupled);
  for (size_t b = 0; b + 1 < l.bptr.size(); ++b) {
    const int hi = l.blk[2 * b], lo = l.blk[2 * b + 1];
    REQUIRE(hi > lo && lo >= 0 && hi < l.N);
    if (b) REQUIRE(l.blk[2 * b - 2] < hi || (l.blk[2 * b - 2] == hi && l.blk[2 * b - 1] < lo));
    REQUIRE(l.bptr[b] < l.bptr[b + 1]);
    for (int q = l.bptr[b]; q < l.bptr[b + 1]; ++q) {
      const int w = l.blist[q], f = w >> 1;
      const int a = l.jk[4 * f + 2], c = l.jk[4 * f + 3];
      REQUIRE((w & 1) == (a < c) && std::max(a, c) == hi && std::min(a, c) == lo);
      if (q > l.bptr[b]) REQUIRE((l.blist[q - 1] >> 1) < f);
    }
  }
  for (int ppt : {5, 10}) {
    int ncb = 0;
    std::vector<uint8_t> adj;
    ba::pgraph_tile_adjacency(l, ppt, &ncb, &adj);
    REQUIRE(ncb == std::max(1, (l.N + ppt - 1) / ppt) && adj.size() == (size_t)ncb * ncb);
    for (int I = 0; I < ncb; ++I) {
      REQUIRE(adj[(size_t)I * ncb + I] == 0);
      for (int J = 0; J < ncb; ++J) REQUIRE(adj[(size_t)I * ncb + J] == adj[(size_t)J * ncb + I]);
    }
    for (size_t b = 0; b + 1 < l.blk.size(); b += 2) {
      const int I = l.blk[b] / ppt, J = l.blk[b + 1] / ppt;
      if (I != J) REQUIRE(adj[(size_t)I * ncb + J] == 1);
    }
  }
  // refusals; the last factor and the last pose are the ones at the arrays' ends
  const int64_t lf = F - 1;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  REQUIRE(ba::pgraph_validate_host(0, T.data(), fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1);
  REQUIRE(ba::pgraph_validate_host(n_pose, T.data(), fixed.data(), 0, j.data(), k.data(), Z.data(), Om.data(), &err) == -1);
  REQUIRE(ba::pgraph_validate_host(n_pose, nullptr, fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1);
  REQUIRE(ba::pgraph_validate_host(n_pose, T.data(), fixed.data(), F, nullptr, k.data(), Z.data(), Om.data(), &err) == -1);
  const int32_t jl = j[lf];
  j[lf] = n_pose;
  REQUIRE(ba::pgraph_validate_host(n_pose, T.data(), fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1 &&
          err.find("(factor " + std::to_string(lf) + ")") != err.npos);
  j[lf] = jl;
  Om[(size_t)F * 36 - 1] = nan;
  REQUIRE(ba::pgraph_validate_host(n_pose, T.data(), fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1 &&
          err.find("Omega is not finite") != err.npos);
  Om[(size_t)F * 36 - 1] = 2.0;
  T[(size_t)n_pose * 12 - 1] = nan;
  REQUIRE(ba::pgraph_validate_host(n_pose, T.data(), fixed.data(), F, j.data(), k.data(), Z.data(), Om.data(), &err) == -1 &&
          err.find("(pose " + std::to_string(n_pose - 1) + ")") != err.npos);
  T[(size_t)n_pose * 12 - 1] = 0.5;
  // the last pose loses its factors: the factors that name it are pointed elsewhere
  if (n_pose > 3 && !fixed[n_pose - 1]) {
    std::vector<int32_t> j2 = j, k2 = k;
    for (int64_t f = 0; f < F; ++f) {
      if (j2[f] == n_pose - 1) j2[f] = k2[f] == 1 ? 2 : 1;
      if (k2[f] == n_pose - 1) k2[f] = j2[f] == 1 ? 2 : 1;
    }
    REQUIRE(ba::pgraph_validate_host(n_pose, T.data(), nullptr, F, j2.data(), k2.data(), Z.data(), Om.data(), &err) == -1 &&
            err == "pose " + std::to_string(n_pose - 1) + " is optimisable but no factor names it");
  }
  return 0;
}

int main() {
  for (int n_pose : {2, 3, 6, 7, 11, 12, 60, 331})
    for (int n_fixed : {0, 1, 2})
      for (int n_cl : {0, 1, 4, 20})
        if (n_fixed < n_pose && one_case(n_pose, n_fixed, n_cl)) return 1;
  std::printf("PGRAPH HOST CHECK PASSED\n");
  return 0;
}
