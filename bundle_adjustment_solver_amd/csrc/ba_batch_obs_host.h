// ba_batch_obs_host.h — host side of the observation mask and cull of the batched full bundle
// adjustment (ba_batch_set_obs_mask, ba_batch_cull, ba_batch_solve_culled): the
// validation of the options, the user <-> planned permutation of the flags and a host
// restatement of what k_ba_batch_mask_apply writes for one problem.  Plain C++ with no HIP
// call, so that it also builds into a stand-alone program under the host sanitizers
// (tools/batch_obs_host_check.cpp).  Internal.
#ifndef BA_BATCH_OBS_HOST_H_
#define BA_BATCH_OBS_HOST_H_

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace ba {

// Everything ba_batch_cull_check refuses.  e2_max: the largest squared error that stays.
inline int cull_validate_host(const double *e2_max, std::string *err) {
  if (!e2_max) {
    *err = "null cull options";
    return -1;
  }
  if (!std::isfinite(*e2_max) || !(*e2_max > 0.0)) {
    *err = "e2_max must be finite and > 0";
    return -1;
  }
  return 0;
}

// The iteration and row rules of ba_batch_solve_culled: both stages iterate, and with rows the
// capacity per problem holds both stages.
inline int solve_culled_validate_host(int it_first, int it_second, bool rows, int cap, std::string *err) {
  if (it_first <= 0 || it_second <= 0) {
    *err = "both stages need max_num_iterations >= 1";
    return -1;
  }
  if (cap < 0) {
    *err = "cap must be >= 0";
    return -1;
  }
  if (rows && (int64_t)cap < (int64_t)it_first + (int64_t)it_second) {
    *err = "cap = " + std::to_string(cap) + " is less than the iterations of both stages (" +
           std::to_string(it_first) + " + " + std::to_string(it_second) + ")";
    return -1;
  }
  return 0;
}

// flags of one problem from user order into planned order (order[t] = user index of planned t)
inline void obs_flags_to_planned(const std::vector<int32_t> &order, const uint8_t *user, std::vector<uint8_t> *planned) {
  planned->resize(order.size());
  for (size_t t = 0; t < order.size(); ++t) (*planned)[t] = user[order[t]] ? 1 : 0;
}

// ... and back
inline void obs_flags_to_user(const std::vector<int32_t> &order, const std::vector<uint8_t> &planned, uint8_t *user) {
  for (size_t t = 0; t < order.size(); ++t) user[order[t]] = planned[t];
}

// What the mask leaves of ONE problem's planned lists.  In: per planned observation its point,
// its pair (or -1) and its flag; lm_ptr (n_pt + 1); per pose-major entry the planned
// observation (pobs) and the N + 1 pointers.  Out: keep (planned indices of the on
// observations, ascending), per kept observation pair << 1 | last writer (or -1), the new
// lm_ptr, pobs (indices into keep) and pobs_ptr, and per pair whether an on observation
// writes it.
struct MaskedLists {
  std::vector<int32_t> keep, w, lm_ptr, pobs, pobs_ptr;
  std::vector<uint8_t> pair_written;
};

inline void mask_compact_host(int n_pt, int n_pair, const std::vector<int32_t> &obs_pt,
                              const std::vector<int32_t> &obs_pair, const std::vector<uint8_t> &on,
                              const std::vector<int32_t> &lm_ptr, const std::vector<int32_t> &pobs,
                              const std::vector<int32_t> &pobs_ptr, MaskedLists *out) {
  const int n = (int)obs_pt.size();
  std::vector<int32_t> pre((size_t)n + 1, 0);
  for (int t = 0; t < n; ++t) pre[t + 1] = pre[t] + (on[t] ? 1 : 0);
  out->keep.clear();
  out->w.clear();
  out->pair_written.assign((size_t)n_pair, 0);
  for (int t = 0; t < n; ++t) {
    if (!on[t]) continue;
    out->keep.push_back(t);
    const int pid = obs_pair[t];
    if (pid < 0) {
      out->w.push_back(-1);
      continue;
    }
    bool later = false;
    for (int t2 = t + 1; t2 < lm_ptr[obs_pt[t] + 1] && !later; ++t2) later = on[t2] && obs_pair[t2] == pid;
    out->w.push_back(pid << 1 | (later ? 0 : 1));
    out->pair_written[pid] = 1;
  }
  out->lm_ptr.resize((size_t)n_pt + 1);
  for (int q = 0; q <= n_pt; ++q) out->lm_ptr[q] = pre[lm_ptr[q]];
  const int N = (int)pobs_ptr.size() - 1;
  out->pobs.clear();
  out->pobs_ptr.assign((size_t)(N > 0 ? N : 0) + 1, 0);
  for (int j = 0; j < N; ++j) {
    for (int e = pobs_ptr[j]; e < pobs_ptr[j + 1]; ++e)
      if (on[pobs[e]]) out->pobs.push_back(pre[pobs[e]]);
    out->pobs_ptr[j + 1] = (int32_t)out->pobs.size();
  }
}

}  // namespace ba
#endif  // BA_BATCH_OBS_HOST_H_
