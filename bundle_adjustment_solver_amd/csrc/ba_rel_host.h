// ba_rel_host.h — host side of the relative-pose factors, once for the handle path
// (ba_set_relative / ba_update_relative, ba_plan.cpp), the batch path (ba_batch_set_relative)
// and the pose graph (ba_pgraph_*): the rules for the caller's arrays, the packing of the
// values the device reads, and the per-pose and per-block factor lists.  Plain C++ with no
// HIP call, so that it also builds into a stand-alone program under the host sanitizers
// (tools/relative_host_check.cpp).  Internal.
#ifndef BA_REL_HOST_H_
#define BA_REL_HOST_H_

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace ba {

// Everything ba_relative_check, ba_pgraph_check and ba_batch_relative_check refuse about the
// factors; *err names the factor, after `where` ("problem 3, " for a batch).  pose_fixed may be
// null (no fixed pose).
// what: kRelPairs — rel_j / rel_k against the poses; kRelValues — Z12 / Omega36 finite;
// kRelNoPoseOk — n_pose < 1 is no error of its own (a batch problem may have no pose: a factor
// of it fails the range rule).  ba_set_relative checks pairs and values, ba_update_relative the
// values (the pairs are the handle's), ba_finalize the pairs again (the poses may have been set anew).
constexpr int kRelPairs = 1, kRelValues = 2, kRelNoPoseOk = 4;
inline int relative_validate_host(int what, int n_pose, const uint8_t *pose_fixed, int64_t n_rel,
                                  const int32_t *rel_j, const int32_t *rel_k, const double *Z12,
                                  const double *Omega36, std::string *err, const std::string &where = "") {
  auto bad = [&](const std::string &m) {
    *err = m;
    return -1;
  };
  if (n_rel < 0) return bad("n_rel must be >= 0");
  if (n_rel >= ((int64_t)1 << 30)) return bad("too many factors for int32 list entries");
  if (n_rel == 0) return 0;
  if ((what & kRelPairs) && !(what & kRelNoPoseOk) && n_pose < 1) return bad("n_pose must be >= 1");
  if (((what & kRelPairs) && (!rel_j || !rel_k)) || ((what & kRelValues) && (!Z12 || !Omega36)))
    return bad("null factor array (" + where + "factor 0)");
  for (int64_t f = 0; f < n_rel; ++f) {
    const std::string at = " (" + where + "factor " + std::to_string(f) + ")";
    if (what & kRelPairs) {
      const int j = rel_j[f], k = rel_k[f];
      if (j < 0 || j >= n_pose) return bad("pose j = " + std::to_string(j) + " out of range" + at);
      if (k < 0 || k >= n_pose) return bad("pose k = " + std::to_string(k) + " out of range" + at);
      if (j == k) return bad("j == k: a factor needs two distinct poses" + at);
      if (pose_fixed && pose_fixed[j] && pose_fixed[k]) return bad("both poses are fixed" + at);
    }
    if (what & kRelValues) {
      for (int e = 0; e < 12; ++e)
        if (!std::isfinite(Z12[12 * f + e])) return bad("Z is not finite" + at);
      for (int e = 0; e < 36; ++e)
        if (!std::isfinite(Omega36[36 * f + e])) return bad("Omega is not finite" + at);
    }
  }
  return 0;
}

// Omega as the device reads it: the lower triangle of O mirrored into the upper one
inline void relative_mirror_omega(const double *O, double *out36) {
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) out36[r * 6 + c] = r >= c ? O[r * 6 + c] : O[c * 6 + r];
}

// The values of the factors as the handle path and the pose graph read them: 48 doubles per
// factor, Z (12) and then the mirrored Omega (36).
constexpr int kRelVal = 48;
inline void relative_pack_values(int64_t n_rel, const double *Z12, const double *Omega36, std::vector<double> *out) {
  out->resize((size_t)n_rel * kRelVal);
  for (int64_t f = 0; f < n_rel; ++f) {
    double *v = out->data() + (size_t)f * kRelVal;
    std::memcpy(v, Z12 + 12 * f, 12 * sizeof(double));
    relative_mirror_omega(Omega36 + 36 * f, v + 12);
  }
}

// The lists the device walks, for validated factors; every list keeps the input order.
struct RelLists {
  std::vector<int32_t> jk;            // 4 per factor: {pose j, pose k, optimisable index of j or -1, of k or -1}
  std::vector<int32_t> pptr, plist;   // per optimisable pose: factor << 1 | (1: it is the factor's k)
  std::vector<int64_t> bkey;          // per coupled block (both poses optimisable): its key, ascending
  std::vector<int32_t> bptr, blist;   // per coupled block: factor << 1 | the key's transposed bit
};

// opt_of_pose: per pose named by rel_j / rel_k, its index among the N optimisable poses or -1.
// key_of(a, b) -> {key of the block that couples the optimisable poses a and b (the same for
// (b, a)), whether the factor's H_jk lies transposed in it}: the caller's block numbering.
template <class KeyOf>
inline void relative_build_lists(int64_t n_rel, const int32_t *rel_j, const int32_t *rel_k, int N,
                                 const int32_t *opt_of_pose, KeyOf key_of, RelLists *out) {
  RelLists &l = *out;
  l = RelLists();
  l.jk.resize((size_t)n_rel * 4);
  l.pptr.assign((size_t)N + 1, 0);
  std::vector<std::pair<int64_t, int32_t>> by_blk;  // (key, factor << 1 | transposed)
  for (int64_t f = 0; f < n_rel; ++f) {
    const int32_t a = opt_of_pose[rel_j[f]], b = opt_of_pose[rel_k[f]];
    int32_t *r = &l.jk[(size_t)f * 4];
    r[0] = rel_j[f];
    r[1] = rel_k[f];
    r[2] = a;
    r[3] = b;
    if (a >= 0) l.pptr[a + 1]++;
    if (b >= 0) l.pptr[b + 1]++;
    if (a >= 0 && b >= 0) {
      const std::pair<int64_t, bool> kb = key_of(a, b);
      by_blk.push_back({kb.first, (int32_t)(f << 1) | (kb.second ? 1 : 0)});
    }
  }
  for (int j = 0; j < N; ++j) l.pptr[j + 1] += l.pptr[j];
  l.plist.resize((size_t)l.pptr[N]);
  std::vector<int32_t> cur(l.pptr.begin(), l.pptr.end() - 1);
  for (int64_t f = 0; f < n_rel; ++f) {
    const int32_t *r = &l.jk[(size_t)f * 4];
    if (r[2] >= 0) l.plist[cur[r[2]]++] = (int32_t)(f << 1);
    if (r[3] >= 0) l.plist[cur[r[3]]++] = (int32_t)(f << 1) | 1;
  }
  std::stable_sort(by_blk.begin(), by_blk.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
  for (size_t t = 0; t < by_blk.size(); ++t) {
    if (t == 0 || by_blk[t].first != by_blk[t - 1].first) {
      l.bkey.push_back(by_blk[t].first);
      l.bptr.push_back((int32_t)t);
    }
    l.blist.push_back(by_blk[t].second);
  }
  l.bptr.push_back((int32_t)by_blk.size());
}

}  // namespace ba
#endif  // BA_REL_HOST_H_
