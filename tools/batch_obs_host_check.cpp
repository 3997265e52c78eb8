// batch_obs_host_check.cpp — stand-alone check of the host side of the observation mask and
// cull of the batched full bundle adjustment (csrc/ba_batch_obs_host.h): the validation of the
// options, the user <-> planned permutation of the flags, and the compaction of one problem's
// lists against a brute-force statement (the lists a fresh plan of the kept observations has).
// No GPU, no HIP, no Python.  Build and run under the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/batch_obs_host_check.cpp -o batch_obs_host_check && ./batch_obs_host_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <random>

#include "../bundle_adjustment_solver_amd/csrc/ba_batch_obs_host.h"

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

namespace {

// the planned lists of one problem, stated directly (ba_batch_create's plan_problem restated):
// stable landmark-major order; a pair per (optimisable landmark, optimisable pose) in (landmark,
// pose) order; the pose-major index
struct Plan {
  std::vector<int32_t> order, obs_pt, obs_pose, obs_pair, lm_ptr, pobs, pobs_ptr;
  std::vector<uint8_t> last;
  int n_pair = 0;
};

Plan plan(int n_pose, const std::vector<uint8_t> &pose_fixed, int n_pt, const std::vector<uint8_t> &pt_fixed,
          const std::vector<int32_t> &u_pose, const std::vector<int32_t> &u_pt) {
  Plan pl;
  const int n = (int)u_pt.size();
  std::vector<int32_t> jopt(n_pose, -1);
  int N = 0;
  for (int p = 0; p < n_pose; ++p)
    if (!pose_fixed[p]) jopt[p] = N++;
  pl.order.resize(n);
  for (int k = 0; k < n; ++k) pl.order[k] = k;
  std::stable_sort(pl.order.begin(), pl.order.end(), [&](int a, int b) { return u_pt[a] < u_pt[b]; });
  pl.lm_ptr.assign(n_pt + 1, 0);
  for (int k = 0; k < n; ++k) pl.lm_ptr[u_pt[k] + 1]++;
  for (int q = 0; q < n_pt; ++q) pl.lm_ptr[q + 1] += pl.lm_ptr[q];
  std::map<std::pair<int, int>, int> pairs;
  for (int t = 0; t < n; ++t) {
    const int q = u_pt[pl.order[t]], j = jopt[u_pose[pl.order[t]]];
    if (!pt_fixed[q] && j >= 0) pairs[{q, j}] = 0;
  }
  for (auto &kv : pairs) kv.second = pl.n_pair++;
  pl.obs_pt.resize(n);
  pl.obs_pose.resize(n);
  pl.obs_pair.assign(n, -1);
  pl.last.assign(n, 0);
  std::map<int, int> writer;
  for (int t = 0; t < n; ++t) {
    pl.obs_pt[t] = u_pt[pl.order[t]];
    pl.obs_pose[t] = u_pose[pl.order[t]];
    const int j = jopt[pl.obs_pose[t]];
    if (!pt_fixed[pl.obs_pt[t]] && j >= 0) {
      pl.obs_pair[t] = pairs[{pl.obs_pt[t], j}];
      writer[pl.obs_pair[t]] = t;  // the last one stays
    }
  }
  for (auto &kv : writer) pl.last[kv.second] = 1;
  pl.pobs_ptr.assign(N + 1, 0);
  for (int j = 0; j < N; ++j) {
    for (int t = 0; t < n; ++t)
      if (jopt[pl.obs_pose[t]] == j) pl.pobs.push_back(t);
    pl.pobs_ptr[j + 1] = (int32_t)pl.pobs.size();
  }
  return pl;
}

void check_problem(std::mt19937 &rng, int n_pose, int n_pt, int n_obs, double p_off) {
  std::vector<uint8_t> pose_fixed(n_pose), pt_fixed(n_pt);
  for (auto &f : pose_fixed) f = rng() % 4 == 0;
  for (auto &f : pt_fixed) f = rng() % 7 == 0;
  std::vector<int32_t> u_pose(n_obs), u_pt(n_obs);
  for (int k = 0; k < n_obs; ++k) {
    u_pose[k] = (int32_t)(rng() % n_pose);
    u_pt[k] = (int32_t)(rng() % n_pt);  // several observations of one pair happen
  }
  std::vector<uint8_t> user(n_obs);
  std::bernoulli_distribution off(p_off);
  for (auto &f : user) f = off(rng) ? 0 : 3;  // any non-zero byte is on
  const Plan full = plan(n_pose, pose_fixed, n_pt, pt_fixed, u_pose, u_pt);

  std::vector<uint8_t> on;
  ba::obs_flags_to_planned(full.order, user.data(), &on);
  std::vector<uint8_t> back(n_obs, 9);
  ba::obs_flags_to_user(full.order, on, back.data());
  for (int k = 0; k < n_obs; ++k) CHECK(back[k] == (user[k] ? 1 : 0));

  ba::MaskedLists m;
  ba::mask_compact_host(n_pt, full.n_pair, full.obs_pt, full.obs_pair, on, full.lm_ptr, full.pobs, full.pobs_ptr, &m);

  // the fresh plan of the kept observations, user order kept
  std::vector<int32_t> k_pose, k_pt, k_user;
  for (int k = 0; k < n_obs; ++k)
    if (user[k]) {
      k_pose.push_back(u_pose[k]);
      k_pt.push_back(u_pt[k]);
      k_user.push_back(k);
    }
  const Plan fresh = plan(n_pose, pose_fixed, n_pt, pt_fixed, k_pose, k_pt);
  const int nk = (int)k_user.size();
  CHECK((int)m.keep.size() == nk && (int)m.w.size() == nk);
  CHECK(m.lm_ptr == fresh.lm_ptr);
  CHECK(m.pobs == fresh.pobs && m.pobs_ptr == fresh.pobs_ptr);
  std::vector<uint8_t> written(full.n_pair, 0);
  for (int t = 0; t < nk; ++t) {
    CHECK(full.order[m.keep[t]] == k_user[fresh.order[t]]);  // the same observation at the same place
    CHECK((m.w[t] < 0) == (fresh.obs_pair[t] < 0));
    if (m.w[t] < 0) continue;
    CHECK((m.w[t] >> 1) == full.obs_pair[m.keep[t]]);   // pair ids stay those of the full structure
    CHECK((m.w[t] & 1) == fresh.last[t]);               // the last writer among the on observations
    written[m.w[t] >> 1] = 1;
  }
  CHECK(written == m.pair_written);
  int live = 0;
  for (uint8_t w : written) live += w;
  CHECK(live == fresh.n_pair);  // a pair without on observation is no pair of the fresh plan
}

}  // namespace

int main() {
  std::string err;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  for (double bad : {nan, inf, -inf, 0.0, -1.0}) {
    err.clear();
    CHECK(ba::cull_validate_host(&bad, &err) == -1 && err.find("e2_max") != std::string::npos);
  }
  CHECK(ba::cull_validate_host(nullptr, &err) == -1 && err == "null cull options");
  const double ok = 25e-4;
  CHECK(ba::cull_validate_host(&ok, &err) == 0);
  CHECK(ba::solve_culled_validate_host(5, 6, true, 11, &err) == 0);
  CHECK(ba::solve_culled_validate_host(5, 6, false, 0, &err) == 0);
  CHECK(ba::solve_culled_validate_host(5, 6, true, 10, &err) == -1 && err.find("cap = 10") != std::string::npos);
  CHECK(ba::solve_culled_validate_host(0, 6, true, 20, &err) == -1);
  CHECK(ba::solve_culled_validate_host(5, -1, false, 0, &err) == -1);
  CHECK(ba::solve_culled_validate_host(5, 6, false, -1, &err) == -1);
  CHECK(ba::solve_culled_validate_host(2000000000, 2000000000, true, 2147483647, &err) == -1);  // no int overflow

  std::mt19937 rng(12345);
  check_problem(rng, 1, 1, 0, 0.5);   // no observations
  check_problem(rng, 3, 4, 40, 1.0);  // everything off
  check_problem(rng, 3, 4, 40, 0.0);  // everything on: the identity
  for (int rep = 0; rep < 200; ++rep)
    check_problem(rng, 1 + (int)(rng() % 9), 1 + (int)(rng() % 30), (int)(rng() % 600), 0.05 + 0.9 * (rep % 5) / 4.0);
  std::printf("BATCH OBS HOST CHECK PASSED\n");
  return 0;
}
