// ba_rel_host.h — host side of the relative-pose factors of the handle path
// (ba_set_relative / ba_update_relative, ba_rel.hip): validation of the caller's arrays and
// packing of the values the device reads.  Plain C++ with no HIP call, so that it also
// builds into a stand-alone program under the host sanitizers
// (tools/relative_host_check.cpp).  Internal.
#ifndef BA_REL_HOST_H_
#define BA_REL_HOST_H_

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace ba {

// Everything ba_relative_check refuses, with the rules and the wording of
// ba_batch_set_relative; *err names the factor.  pose_fixed may be null (no fixed pose).
// what: kRelPairs — rel_j / rel_k against the poses; kRelValues — Z12 / Omega36 finite.
// ba_set_relative checks both, ba_update_relative the values (the pairs are the handle's),
// ba_finalize the pairs again (the poses may have been set anew).
constexpr int kRelPairs = 1, kRelValues = 2;
inline int relative_validate_host(int what, int n_pose, const uint8_t *pose_fixed, int64_t n_rel,
                                  const int32_t *rel_j, const int32_t *rel_k, const double *Z12,
                                  const double *Omega36, std::string *err) {
  auto bad = [&](const std::string &m) {
    *err = m;
    return -1;
  };
  if (n_rel < 0) return bad("n_rel must be >= 0");
  if (n_rel >= ((int64_t)1 << 30)) return bad("too many factors for int32 list entries");
  if (n_rel == 0) return 0;
  if ((what & kRelPairs) && n_pose < 1) return bad("n_pose must be >= 1");
  if (((what & kRelPairs) && (!rel_j || !rel_k)) || ((what & kRelValues) && (!Z12 || !Omega36)))
    return bad("null factor array (factor 0)");
  for (int64_t f = 0; f < n_rel; ++f) {
    const std::string at = " (factor " + std::to_string(f) + ")";
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

// The values of the factors as the device reads them: 48 doubles per factor, Z (12) and then
// Omega (36) with the lower triangle mirrored into the upper one.
constexpr int kRelVal = 48;
inline void relative_pack_values(int64_t n_rel, const double *Z12, const double *Omega36, std::vector<double> *out) {
  out->resize((size_t)n_rel * kRelVal);
  for (int64_t f = 0; f < n_rel; ++f) {
    double *v = out->data() + (size_t)f * kRelVal;
    std::memcpy(v, Z12 + 12 * f, 12 * sizeof(double));
    const double *O = Omega36 + 36 * f;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) v[12 + r * 6 + c] = r >= c ? O[r * 6 + c] : O[c * 6 + r];
  }
}

}  // namespace ba
#endif  // BA_REL_HOST_H_
