// ba_plan.cpp — see ba_plan.h.  Host-only, no HIP.
#include "ba_plan.h"

#include "ba_dense_sched.h"
#include "ba_rel_host.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <limits>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <thread>

#include <sys/mman.h>

namespace ba {

void *plan_big_alloc(size_t bytes) {
  void *p = nullptr;
  const size_t sz = (bytes + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1);
  if (posix_memalign(&p, (size_t)2 << 20, sz) != 0 || !p) throw std::bad_alloc();
  (void)madvise(p, sz, MADV_HUGEPAGE);  // advisory: plain pages when THP is off
  return p;
}
void plan_big_free(void *p, size_t) { free(p); }

namespace {

// PlanKnobs::times: wall time of the planner's phases on stderr (developer knob)
struct PhaseClock {
  const bool on;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void lap(const char *what) {
    if (!on) return;
    const auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "[plan] %-28s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(n - t).count());
    t = n;
  }
};

// Host threads of the planner: PlanKnobs::threads, or the hardware's, at most 16.
int plan_threads(int knob) {
  return knob > 0 ? knob : std::max(1, std::min((int)std::thread::hardware_concurrency(), 16));
}
// Static-chunk parallel loop over [0, n) on at most `threads` host threads.  Every use
// below writes disjoint outputs per index and all prefix sums stay sequential, so the
// plan is identical for every thread count (tests/cpp/plan_check.cpp compares it with
// the one-thread build).
// (grain: indices a thread should at least get — 4096 for per-landmark loops; loops over
//  runs / buckets of hundreds of landmarks pass a small one)
template <class F>
void parallel_for(int threads, int64_t n, const F &fn, int64_t grain = 4096) {
  const int nt = (int)std::min<int64_t>(threads, std::max<int64_t>(1, n / grain));
  if (nt <= 1) {
    fn((int64_t)0, n);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&, t] { fn(n * t / nt, n * (t + 1) / nt); });
  for (auto &x : th) x.join();
}

// Internal pose order: optimised poses in input order, then fixed poses.
void order_poses(const PlanInput &in, std::vector<int32_t> &int_of_user,
                 std::vector<int32_t> &user_of_int,
                 std::vector<int32_t> &jopt_of_user, int &N) {
  int_of_user.assign(in.n_pose, -1);
  user_of_int.clear();
  jopt_of_user.assign(in.n_pose, -1);
  N = 0;
  for (int p = 0; p < in.n_pose; ++p)
    if (!in.pose_fixed[p]) {
      jopt_of_user[p] = N;
      int_of_user[p] = N++;
      user_of_int.push_back(p);
    }
  int nxt = N;
  for (int p = 0; p < in.n_pose; ++p)
    if (in.pose_fixed[p]) {
      int_of_user[p] = nxt++;
      user_of_int.push_back(p);
    }
}

// Locality order of all points: (first observing internal pose, input index).
void locality_order(const PlanInput &in, int threads,
                    const std::vector<int32_t> &pose_int_of_user,
                    std::vector<int32_t> &order,
                    std::vector<int64_t> &obs_count) {
  std::vector<int32_t> first_pose(in.n_pt, in.n_pose);
  obs_count.assign(in.n_pt, 0);
  // (threaded by point range: every thread scans the whole list and keeps its own points)
  parallel_for(threads, in.n_pt, [&](int64_t q0, int64_t q1) {
    for (int64_t k = 0; k < in.n_obs; ++k) {
      const int64_t q = in.obs_pt[k];
      if (q < q0 || q >= q1) continue;
      const int j = pose_int_of_user[in.obs_pose[k]];
      if (j < first_pose[q]) first_pose[q] = j;
      obs_count[q]++;
    }
  });
  // counting sort by first_pose keeps input index order inside a bucket
  std::vector<int64_t> bucket(in.n_pose + 2, 0);
  for (int q = 0; q < in.n_pt; ++q) bucket[first_pose[q] + 1]++;
  for (int b = 0; b <= in.n_pose; ++b) bucket[b + 1] += bucket[b];
  order.resize(in.n_pt);
  for (int q = 0; q < in.n_pt; ++q) order[bucket[first_pose[q]]++] = q;
}

// Landmarks per Schur super-run for a shard of M optimised landmarks: the kernel
// runs kSchurRunTarget workgroups at a time, so the runs are sized to fill a
// whole number of such rounds (C4: 500 k landmarks -> 2 rounds of 326 instead
// of 2.5 rounds of 256), at most kSchurSuperLandmarks and at least
// kSchurSuperMin each.
int schur_run_cap(int64_t M, int knob) {
  const int64_t rounds = std::max<int64_t>(
      1, (M + (int64_t)kSchurRunTarget * kSchurSuperLandmarks - 1) /
             ((int64_t)kSchurRunTarget * kSchurSuperLandmarks));
  if (knob > 0) return knob;  // PlanKnobs::sup_cap (tuning knob)
  return (int)std::min<int64_t>(
      kSchurSuperLandmarks,
      std::max<int64_t>(kSchurSuperMin,
                        (M + kSchurRunTarget * rounds - 1) / (kSchurRunTarget * rounds)));
}

void assign_owner(const PlanInput &in, const std::vector<int32_t> &order,
                  const std::vector<int64_t> &obs_count,
                  std::vector<int32_t> &owner) {
  owner.assign(in.n_pt, 0);
  if (in.world <= 1) return;
  // weight = observations + 1 so that unobserved points are spread too
  const long double total = (long double)in.n_obs + (long double)in.n_pt;
  long double cum = 0;
  for (int idx = 0; idx < in.n_pt; ++idx) {
    const int q = order[idx];
    int r = (int)((cum * in.world) / total);
    if (r >= in.world) r = in.world - 1;
    owner[q] = r;
    cum += (long double)obs_count[q] + 1;
  }
}

void make_chunks(const std::vector<int64_t> &ptr, int n_seg, int chunk,
                 std::vector<int32_t> &c_seg, std::vector<int64_t> &c_begin,
                 std::vector<int64_t> &c_end, std::vector<int32_t> &seg_cptr) {
  c_seg.clear();
  c_begin.clear();
  c_end.clear();
  seg_cptr.assign(n_seg + 1, 0);
  for (int s = 0; s < n_seg; ++s) {
    const int64_t len = ptr[s + 1] - ptr[s];
    if (len > 0) {
      // equal pieces (multiples of 64 so that a wave's last step is full)
      const int64_t nc = (len + chunk - 1) / chunk;
      int64_t piece = (len + nc - 1) / nc;
      piece = std::min<int64_t>((piece + 63) / 64 * 64, chunk);
      for (int64_t b = ptr[s]; b < ptr[s + 1]; b += piece) {
        c_seg.push_back(s);
        c_begin.push_back(b);
        c_end.push_back(std::min<int64_t>(b + piece, ptr[s + 1]));
      }
    }
    seg_cptr[s + 1] = (int32_t)c_seg.size();
  }
}

}  // namespace

// Lane table of one Schur super-run (k_schur_lds: 4 waves x 64 lanes).  Slot s
// gets an even number of lanes n_s in [2, 32], contiguous inside ONE wave, in
// proportion to its triple count; lane word = slot | h << 8 | sub2 << 9 |
// (n_s / 2) << 14, 0xff = idle lane.  Waves: longest-processing-time first on
// the triple counts; lanes inside a wave: repeatedly +2 to the slot with the
// most triples per lane.  Deterministic (ties by slot id).
void deal_lanes(const std::vector<int64_t> &tcount, std::vector<uint32_t> &out) {
  const int ns = (int)tcount.size();
  std::vector<int> ord(ns);
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return tcount[a] > tcount[b]; });
  std::vector<int> wave_of(ns, 0), nl(ns, 2);
  int64_t load[4] = {0, 0, 0, 0};
  int cnt[4] = {0, 0, 0, 0};
  for (int s : ord) {
    int w = -1;
    for (int c = 0; c < 4; ++c)
      if (cnt[c] < 32 && (w < 0 || load[c] < load[w])) w = c;
    wave_of[s] = w;
    load[w] += tcount[s];
    cnt[w]++;
  }
  const size_t base = out.size();
  out.resize(base + 256, 0xffu);
  for (int w = 0; w < 4; ++w) {
    int free_lanes = 64 - 2 * cnt[w];
    while (free_lanes >= 2) {
      int best = -1;
      for (int s = 0; s < ns; ++s) {
        if (wave_of[s] != w || nl[s] >= 32) continue;
        // tcount[s] / nl[s] > tcount[best] / nl[best], in integers
        if (best < 0 || tcount[s] * nl[best] > tcount[best] * nl[s]) best = s;
      }
      if (best < 0 || tcount[best] == 0) break;
      nl[best] += 2;
      free_lanes -= 2;
    }
    int lane = 0;
    for (int s = 0; s < ns; ++s) {
      if (wave_of[s] != w) continue;
      for (int sub = 0; sub < nl[s]; ++sub)
        out[base + 64 * w + lane + sub] =
            (uint32_t)s | ((uint32_t)(sub & 1) << 8) | ((uint32_t)(sub >> 1) << 9) |
            ((uint32_t)(nl[s] >> 1) << 14);
      lane += nl[s];
    }
  }
}

void partition_points(const PlanInput &in, int threads, std::vector<int32_t> &owner) {
  std::vector<int32_t> piu, pui, jou;
  int N = 0;
  order_poses(in, piu, pui, jou, N);
  std::vector<int32_t> order;
  std::vector<int64_t> cnt;
  locality_order(in, plan_threads(threads), piu, order, cnt);
  assign_owner(in, order, cnt, owner);
}

// ======================================================================================
// build_plan, phase by phase.  Every phase is a function whose signature shows what it
// reads (const) and what it fills; build_plan at the end of the file calls them in order.
// ======================================================================================
namespace {

// ---- input checks ----
std::string check_sizes(const PlanInput &in) {
  if (in.n_cam <= 0) return "no cameras";
  if (in.n_pose <= 0) return "no poses";
  if (in.n_pt <= 0) return "no points";
  if (in.world < 1 || in.rank < 0 || in.rank >= in.world) return "bad rank/world";
  return std::string();
}

bool bad_camera(const PlanInput &in, int64_t k) { return in.obs_cam[k] < 0 || in.obs_cam[k] >= in.n_cam; }
bool bad_pose(const PlanInput &in, int64_t k) { return in.obs_pose[k] < 0 || in.obs_pose[k] >= in.n_pose; }
bool bad_point(const PlanInput &in, int64_t k) { return in.obs_pt[k] < 0 || in.obs_pt[k] >= in.n_pt; }

// The first offending observation (the smallest index, whatever the thread count) and,
// on it, camera before pose before point.
std::string validate_observations(const PlanInput &in, int threads) {
  std::vector<int64_t> bad((size_t)threads + 1, INT64_MAX);
  std::atomic<int> slot{0};
  parallel_for(threads, in.n_obs, [&](int64_t k0, int64_t k1) {
    const int me = slot.fetch_add(1);
    for (int64_t k = k0; k < k1; ++k)
      if (bad_camera(in, k) || bad_pose(in, k) || bad_point(in, k)) {
        bad[me] = k;
        break;
      }
  });
  const int64_t k = *std::min_element(bad.begin(), bad.end());
  if (k == INT64_MAX) return std::string();
  if (bad_camera(in, k)) return "observation with invalid camera index";
  if (bad_pose(in, k)) return "observation with invalid pose index";
  return "observation with invalid point index";
}

// ---- points: global opt index (input order), locality order, owners ----
// The owned points with pt_fixed == `fixed`, in locality order, get the next internal indices.
void append_owned_points(const PlanInput &in, const std::vector<int32_t> &order, bool fixed, Plan &pl) {
  for (int idx = 0; idx < in.n_pt; ++idx) {
    const int q = order[idx];
    if (pl.owner[q] == in.rank && (in.pt_fixed[q] != 0) == fixed) {
      pl.pt_int_of_user[q] = (int32_t)pl.pt_user_of_int.size();
      pl.pt_user_of_int.push_back(q);
    }
  }
}

// Fills iopt_of_user / M_global, owner, and the optimised part of pt_user_of_int /
// pt_int_of_user (M landmarks, preliminary: locality order).  Returns the locality order
// of ALL points, which append_fixed_points needs again.
std::vector<int32_t> number_points(const PlanInput &in, int threads, Plan &pl) {
  pl.iopt_of_user.assign(in.n_pt, -1);
  pl.M_global = 0;
  for (int q = 0; q < in.n_pt; ++q)
    if (!in.pt_fixed[q]) pl.iopt_of_user[q] = pl.M_global++;
  std::vector<int32_t> order;
  std::vector<int64_t> cnt;
  locality_order(in, threads, pl.pose_int_of_user, order, cnt);
  assign_owner(in, order, cnt, pl.owner);
  pl.pt_int_of_user.assign(in.n_pt, -1);
  append_owned_points(in, order, false, pl);
  pl.M = (int)pl.pt_user_of_int.size();
  return order;
}

// ---- observations of the OWNED points as a CSR over user point ids, every list in
// (pose, insertion) order: built once, used by the covisibility grouping and, landmark by
// landmark in the final order, by the landmark-major list ----
// (packed records: every later pass reads a landmark's observations as ONE contiguous
//  run instead of gathering four input arrays at random positions)
struct ObsRecP {
  int32_t pose, cam;  // internal pose index, camera
  double u, v;
};
struct PointObs {
  std::vector<int64_t> ptr;  // n_pt + 1, by USER point id
  pvec<ObsRecP> rec;
  int64_t begin(int q) const { return ptr[q]; }
  int64_t end(int q) const { return ptr[q + 1]; }
  int64_t count(int q) const { return ptr[q + 1] - ptr[q]; }
};

// stable insertion sort by pose (lists are short and nearly sorted: the usual insertion
// order is pose-major)
void sort_by_pose(ObsRecP *a, int64_t n) {
  for (int64_t i = 1; i < n; ++i) {
    if (a[i - 1].pose <= a[i].pose) continue;
    const ObsRecP x = a[i];
    int64_t j = i;
    while (j > 0 && a[j - 1].pose > x.pose) {
      a[j] = a[j - 1];
      --j;
    }
    a[j] = x;
  }
}

// (counting sort by point id, threaded by POINT RANGE: every thread scans the whole
//  observation list — a sequential read — and files the observations of its own points,
//  in input order: the result does not depend on the thread count)
PointObs build_point_obs(const PlanInput &in, int threads, const Plan &pl) {
  PointObs po;
  po.ptr.assign((size_t)in.n_pt + 1, 0);
  parallel_for(threads, in.n_pt, [&](int64_t q0, int64_t q1) {
    for (int64_t k = 0; k < in.n_obs; ++k) {
      const int64_t q = in.obs_pt[k];
      if (q >= q0 && q < q1 && pl.owner[q] == in.rank) po.ptr[q + 1]++;
    }
  });
  for (int q = 0; q < in.n_pt; ++q) po.ptr[q + 1] += po.ptr[q];
  po.rec.resize((size_t)po.ptr[in.n_pt]);
  pvec<int64_t> cur((size_t)in.n_pt);
  parallel_for(threads, in.n_pt, [&](int64_t q0, int64_t q1) {
    for (int64_t q = q0; q < q1; ++q) cur[q] = po.ptr[q];
    for (int64_t k = 0; k < in.n_obs; ++k) {
      const int64_t q = in.obs_pt[k];
      if (q < q0 || q >= q1 || pl.owner[q] != in.rank) continue;
      ObsRecP &r = po.rec[cur[q]++];
      r.pose = pl.pose_int_of_user[in.obs_pose[k]];
      r.cam = in.obs_cam[k];
      r.u = in.obs_uv ? in.obs_uv[2 * k + 0] : 0.0;
      r.v = in.obs_uv ? in.obs_uv[2 * k + 1] : 0.0;
    }
  });
  parallel_for(threads, in.n_pt, [&](int64_t q0, int64_t q1) {
    for (int64_t q = q0; q < q1; ++q) sort_by_pose(po.rec.data() + po.ptr[q], po.ptr[q + 1] - po.ptr[q]);
  });
  return po;
}

// ---- covisibility groups: landmarks with the identical OBSERVATION PATTERN —
// the same sequence of (pose, camera) over their observations in landmark-major
// order, fixed poses included — hence the identical set of optimisable poses
// (1..kGrpMaxPoses of them), in groups of >= kGrpMinLandmarks come FIRST, group
// after group (groups ordered by their patterns, i.e. still by first observing
// pose; landmarks of a group in locality order).  k_lin_grp linearises a group
// with one lane per pattern slot (pose and camera are lane constants: no
// gathers, no index records, pose side in the same pass); k_schur_grp turns its
// Schur contributions into one dense product.  Everything else keeps the
// locality order and goes through the chunk / super-run kernels. ----

// distinct optimisable poses (internal index < N) among pattern words sorted by pose
int distinct_opt_poses(const uint64_t *w, const uint64_t *end, int N) {
  int n = 0;
  int64_t last = -1;
  for (; w != end; ++w) {
    const int64_t ji = (int64_t)(*w >> 32);
    if (ji < N && ji != last) ++n;
    last = ji;
  }
  return n;
}

// The pattern of every optimised landmark (preliminary index i): words (pose << 32) |
// camera in (pose, insertion) order.
struct Patterns {
  int N = 0;                // optimised poses
  std::vector<int64_t> kp;  // M + 1
  pvec<uint64_t> pat;
  const uint64_t *begin(int i) const { return pat.data() + kp[i]; }
  const uint64_t *end(int i) const { return pat.data() + kp[i + 1]; }
  int deg(int i) const { return (int)(kp[i + 1] - kp[i]); }
  int dopt(int i) const { return distinct_opt_poses(begin(i), end(i), N); }
  // lexicographic on the patterns, shorter first on ties
  bool less(int a, int b) const {
    const int da = deg(a), db = deg(b);
    for (int t = 0; t < std::min(da, db); ++t)
      if (begin(a)[t] != begin(b)[t]) return begin(a)[t] < begin(b)[t];
    return da < db;
  }
  bool same(int a, int b) const { return deg(a) == deg(b) && std::equal(begin(a), end(a), begin(b)); }
  // a member of a superset group must list its (pose, camera) entries in strictly
  // increasing order: the slots of the union are in that order, and the pair's last
  // WRITER (reference :826: the last inserted observation of a pose) is then the last
  // valid slot of the pose.  (Duplicates and cameras inserted in descending order:
  // exact groups only.)
  bool has_dup(int i) const {
    for (const uint64_t *w = begin(i) + 1; w < end(i); ++w)
      if (w[0] <= w[-1]) return true;
    return false;
  }
};

Patterns build_patterns(const Plan &pl, const PointObs &po, int threads) {
  Patterns pt;
  pt.N = pl.N;
  pt.kp.assign((size_t)pl.M + 1, 0);
  for (int i = 0; i < pl.M; ++i) pt.kp[i + 1] = pt.kp[i] + po.count(pl.pt_user_of_int[i]);
  pt.pat.resize((size_t)pt.kp[pl.M]);
  parallel_for(threads, pl.M, [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
      const int q = pl.pt_user_of_int[i];
      int64_t w = pt.kp[i];
      for (int64_t t = po.begin(q); t < po.end(q); ++t)
        pt.pat[w++] = ((uint64_t)(uint32_t)po.rec[t].pose << 32) | (uint32_t)po.rec[t].cam;
    }
  });
  return pt;
}

// The landmarks that may join a group, and what the group builders ask about every landmark.
struct Candidates {
  std::vector<int32_t> cand;  // preliminary landmark indices, in the order the current step needs
  std::vector<int32_t> dop;   // M: distinct optimisable poses
  // the pose SPAN of a landmark in USER pose indices (the registration order of the
  // poses is normally the trajectory; the internal order puts the fixed poses last,
  // which would throw every window that touches a fixed pose into one bucket)
  std::vector<int32_t> span_lo, span_hi;  // M
  bool same_span(int a, int b) const { return span_lo[a] == span_lo[b] && span_hi[a] == span_hi[b]; }
};

void select_candidates(const Patterns &pt, int M, Candidates &c) {
  c.dop.assign(M, 0);
  for (int i = 0; i < M; ++i) {
    c.dop[i] = pt.dopt(i);
    // (dop == 0: landmarks seen by fixed poses only — the first poses of a trajectory are
    //  usually fixed — have no pair and no Schur term, but they are linearised and
    //  back-substituted: groups of them keep those kernels' chunk launches empty)
    if (c.dop[i] <= kGrpMaxPoses && pt.deg(i) >= 1 && pt.deg(i) <= kGrpMaxObs) c.cand.push_back(i);
  }
}

// stable sort by pattern (stable: locality order inside a group).  The candidates
// arrive in locality order, i.e. already grouped by their first observing pose = the
// first pattern word's pose: every run of equal first pose is sorted on its own, the
// runs in parallel (the result is the stable sort of the whole list whenever the
// first poses are non-decreasing, which the check below establishes).
void sort_by_pattern(const Patterns &pt, int threads, std::vector<int32_t> &cand) {
  const auto less = [&pt](int a, int b) { return pt.less(a, b); };
  std::vector<size_t> run0(1, 0);
  bool monotone = true;
  for (size_t t = 1; t < cand.size(); ++t) {
    const uint64_t a0 = *pt.begin(cand[t - 1]) >> 32, b0 = *pt.begin(cand[t]) >> 32;
    if (b0 < a0) monotone = false;
    if (b0 != a0) run0.push_back(t);
  }
  run0.push_back(cand.size());
  if (!monotone) {
    std::stable_sort(cand.begin(), cand.end(), less);
    return;
  }
  parallel_for(threads, (int64_t)run0.size() - 1, [&](int64_t r0, int64_t r1) {
    for (int64_t r = r0; r < r1; ++r)  // (regular scenes: one pattern per run, nothing to sort)
      if (!std::is_sorted(cand.begin() + run0[r], cand.begin() + run0[r + 1], less))
        std::stable_sort(cand.begin() + run0[r], cand.begin() + run0[r + 1], less);
  }, 8);
}

void pose_spans(const Plan &pl, const Patterns &pt, int threads, Candidates &c) {
  c.span_lo.assign(pl.M, 0);
  c.span_hi.assign(pl.M, 0);
  parallel_for(threads, pl.M, [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
      int32_t lo = INT32_MAX, hi = -1;
      for (const uint64_t *w = pt.begin((int)i); w != pt.end((int)i); ++w) {
        const int32_t u = pl.pose_user_of_int[(size_t)(*w >> 32)];
        lo = std::min(lo, u);
        hi = std::max(hi, u);
      }
      c.span_lo[i] = lo;
      c.span_hi[i] = hi;
    }
  });
}

// ---- groups.  A run of candidates with the IDENTICAL pattern is an exact group.
// SUPERSET groups take what real visibility leaves of that — occlusion, image borders,
// track loss make the patterns of one pose window differ from landmark to landmark: all
// candidates with the same pose SPAN (first and last observing pose) form one group whose
// pattern is the UNION of theirs; a member's missing observations become padded slots
// (uv = NaN: weight 0, no cost) and its missing pairs zero W records, so that the group
// kernels keep their one-lane-per-(landmark, slot) layout.  Landmarks that lost their
// first or last pose altogether join a group whose union contains their pattern.
// (PlanKnobs::superset off: exact groups only; masks need k_lin_grp, so also off without
// PlanKnobs::lin_groups.)
struct GroupBuild {
  std::vector<uint64_t> upat;     // union pattern, sorted
  std::vector<int32_t> members;   // preliminary landmark indices
  int d = 0;
  bool masked = false;
  int32_t first_pose = 0, last_pose = 0;  // span in user pose indices
};
struct Grouping {
  std::vector<GroupBuild> groups;
  std::vector<int32_t> group_of;  // M: group of every landmark or -1
  // numbers the groups of `from` and files their members
  void adopt(std::vector<GroupBuild> &from) {
    for (GroupBuild &gb : from) {
      for (int32_t i : gb.members) group_of[i] = (int32_t)groups.size();
      groups.push_back(std::move(gb));
    }
    from.clear();
  }
};

// (the group builders append to `out`; the caller adopts the groups afterwards: buckets
//  are processed on host threads)
void exact_runs(const Patterns &pt, const Candidates &c, size_t lo, size_t hi, std::vector<GroupBuild> &out) {
  size_t a = lo;
  while (a < hi) {
    size_t b = a + 1;
    while (b < hi && pt.same(c.cand[a], c.cand[b])) ++b;
    if ((int)(b - a) >= kGrpMinLandmarks) {
      GroupBuild gb;
      gb.upat.assign(pt.begin(c.cand[a]), pt.end(c.cand[a]));
      gb.d = c.dop[c.cand[a]];
      gb.first_pose = c.span_lo[c.cand[a]];
      gb.last_pose = c.span_hi[c.cand[a]];
      gb.members.assign(c.cand.begin() + a, c.cand.begin() + b);
      out.push_back(std::move(gb));
    }
    a = b;
  }
}

// buckets of equal (first pose, last pose); inside a bucket the pattern order stays
// (stable, by two counting passes — last pose, then first pose)
void sort_by_span(int n_pose, Candidates &c) {
  std::vector<int32_t> tmp(c.cand.size());
  auto pass = [n_pose](const std::vector<int32_t> &key, const std::vector<int32_t> &src, std::vector<int32_t> &dst) {
    std::vector<int64_t> at((size_t)n_pose + 1, 0);
    for (int32_t i : src) at[(size_t)key[i] + 1]++;
    for (int b = 0; b < n_pose; ++b) at[b + 1] += at[b];
    for (int32_t i : src) dst[at[key[i]]++] = i;
  };
  pass(c.span_hi, c.cand, tmp);
  pass(c.span_lo, tmp, c.cand);
}

// One span bucket cand[a, b): the union of its duplicate-free members' patterns is a
// superset group if it is small and dense enough; otherwise, and among the members with
// duplicate observations, exact runs.  (`uni`: the caller's scratch.)
void bucket_groups(const Patterns &pt, const Candidates &c, size_t a, size_t b, std::vector<uint64_t> &uni,
                   std::vector<GroupBuild> &out) {
  if (pt.same(c.cand[a], c.cand[b - 1])) return exact_runs(pt, c, a, b, out);  // (sorted by pattern: first == last => all equal)
  uni.clear();
  int64_t slots = 0;
  int n_el = 0;
  for (size_t t = a; t < b; ++t) {
    const int i = c.cand[t];
    if (pt.has_dup(i)) continue;
    uni.insert(uni.end(), pt.begin(i), pt.end(i));
    slots += pt.deg(i);
    ++n_el;
  }
  std::sort(uni.begin(), uni.end());
  uni.erase(std::unique(uni.begin(), uni.end()), uni.end());
  const int du = distinct_opt_poses(uni.data(), uni.data() + uni.size(), pt.N);
  if (!(n_el >= kGrpMinLandmarks && (int)uni.size() <= kGrpMaxObs && du <= kGrpMaxPoses &&
        (double)slots >= 0.55 * (double)n_el * (double)uni.size()))
    return exact_runs(pt, c, a, b, out);
  GroupBuild gb;
  gb.upat = uni;
  gb.d = du;
  gb.first_pose = c.span_lo[c.cand[a]];
  gb.last_pose = c.span_hi[c.cand[a]];
  for (size_t t = a; t < b; ++t) {
    const int i = c.cand[t];
    if (pt.has_dup(i)) continue;
    gb.members.push_back(i);
    if (pt.deg(i) < (int)uni.size()) gb.masked = true;
  }
  out.push_back(std::move(gb));
}

// The candidates (sorted by span, then pattern) bucket by bucket, in bucket order.
void superset_buckets(const Patterns &pt, const Candidates &c, int threads, Grouping &g) {
  const std::vector<int32_t> &cand = c.cand;
  std::vector<size_t> bkt(1, 0);  // bucket boundaries
  for (size_t t = 1; t < cand.size(); ++t)
    if (!c.same_span(cand[t], cand[t - 1])) bkt.push_back(t);
  bkt.push_back(cand.size());
  const size_t nbkt = cand.empty() ? 0 : bkt.size() - 1;
  std::vector<std::vector<GroupBuild>> bout(nbkt);
  parallel_for(threads, (int64_t)nbkt, [&](int64_t k0, int64_t k1) {
    std::vector<uint64_t> uni;
    for (int64_t k = k0; k < k1; ++k) bucket_groups(pt, c, bkt[k], bkt[k + 1], uni, bout[k]);
  }, 8);
  for (size_t k = 0; k < nbkt; ++k) g.adopt(bout[k]);
}

// leftovers join a group whose union contains their pattern
void join_leftovers(int n_pose, const Patterns &pt, const Candidates &c, Grouping &g) {
  std::vector<std::vector<int32_t>> by_first((size_t)n_pose + 1);
  for (size_t gidx = 0; gidx < g.groups.size(); ++gidx) by_first[(size_t)g.groups[gidx].first_pose].push_back((int32_t)gidx);
  for (int i : c.cand) {
    if (g.group_of[i] >= 0 || pt.has_dup(i)) continue;
    const int32_t f = c.span_lo[i], l = c.span_hi[i];
    bool joined = false;
    for (int32_t g0 = f; g0 >= 0 && g0 > f - kGrpMaxObs && !joined; --g0)
      for (int32_t gidx : by_first[g0]) {
        GroupBuild &gb = g.groups[gidx];
        if (gb.last_pose < l) continue;
        if (!std::includes(gb.upat.begin(), gb.upat.end(), pt.begin(i), pt.end(i))) continue;
        gb.members.push_back(i);
        g.group_of[i] = gidx;
        if (pt.deg(i) < (int)gb.upat.size()) gb.masked = true;
        joined = true;
        break;
      }
  }
}

// The grouped landmarks first, group after group (grp_range, grp_upat, M_grp), then the
// rest in its old order.
void renumber_by_group(Grouping &g, Plan &pl) {
  const int M0 = pl.M;
  std::vector<int32_t> neworder;
  neworder.reserve(M0);
  for (GroupBuild &gb : g.groups) {
    std::sort(gb.members.begin(), gb.members.end());  // locality order inside a group
    Plan::GrpRange gr;
    gr.l0 = (int32_t)neworder.size();
    gr.nl = (int32_t)gb.members.size();
    gr.d = gb.d;
    gr.no = (int32_t)gb.upat.size();
    gr.masked = gb.masked ? 1 : 0;
    gr.upat0 = (int64_t)pl.grp_upat.size();
    pl.grp_upat.insert(pl.grp_upat.end(), gb.upat.begin(), gb.upat.end());
    pl.grp_range.push_back(gr);
    for (int32_t i : gb.members) neworder.push_back(pl.pt_user_of_int[i]);
  }
  pl.M_grp = (int)neworder.size();
  for (int i = 0; i < M0; ++i)
    if (g.group_of[i] < 0) neworder.push_back(pl.pt_user_of_int[i]);
  pl.pt_user_of_int.swap(neworder);
  for (int k = 0; k < M0; ++k) pl.pt_int_of_user[pl.pt_user_of_int[k]] = k;
}

// The grouping as a whole: sets lin_groups, M_grp, grp_range, grp_upat and reorders the
// optimised landmarks.
void group_landmarks(const PlanInput &in, const PlanKnobs &knobs, int threads, const PointObs &po, PhaseClock &clk, Plan &pl) {
  pl.lin_groups = knobs.lin_groups && pl.n_cam < 65536;  // (the pattern record packs the camera into 16 bits)
  if (pl.M > 0 && knobs.groups) {
    const Patterns pt = build_patterns(pl, po, threads);
    clk.lap("  groups: patterns");
    Candidates c;
    select_candidates(pt, pl.M, c);
    clk.lap("  groups: candidates");
    sort_by_pattern(pt, threads, c.cand);
    clk.lap("  groups: pattern sort");
    pose_spans(pl, pt, threads, c);
    Grouping g;
    g.group_of.assign(pl.M, -1);
    if (!(pl.lin_groups && knobs.superset)) {
      std::vector<GroupBuild> out;
      exact_runs(pt, c, 0, c.cand.size(), out);
      g.adopt(out);
    } else {
      sort_by_span(in.n_pose, c);
      clk.lap("  groups: span sort");
      superset_buckets(pt, c, threads, g);
      clk.lap("  groups: buckets");
      join_leftovers(in.n_pose, pt, c, g);
    }
    clk.lap("  groups: leftovers");
    renumber_by_group(g, pl);
  }
  if (pl.M_grp == 0) pl.lin_groups = false;
}

// Interleave inside windows of one Schur super-run: position p of a window
// takes the landmark p would have had in residue-class order (k = r, r + S,
// r + 2S, ...), so that every chunk of consecutive landmarks samples the
// WHOLE window and touches the run's S blocks in the run's proportions
// (the lanes of the Schur kernel are dealt to the blocks in those proportions).
void interleave_windows(const PlanKnobs &knobs, Plan &pl) {
  const int W = schur_run_cap(pl.M - pl.M_grp, knobs.sup_cap);
  std::vector<int32_t> tmp;
  for (int base = pl.M_grp; base < pl.M; base += W) {
    const int n = std::min(W, pl.M - base);
    tmp.clear();
    for (int r = 0; r < kSchurInterleave; ++r)
      for (int k = r; k < n; k += kSchurInterleave) tmp.push_back(pl.pt_user_of_int[base + k]);
    for (int k = 0; k < n; ++k) pl.pt_user_of_int[base + k] = tmp[k];
  }
  for (int k = 0; k < pl.M; ++k) pl.pt_int_of_user[pl.pt_user_of_int[k]] = k;
}

// the owned fixed points behind the optimised ones: n_pt
void append_fixed_points(const PlanInput &in, const std::vector<int32_t> &order, Plan &pl) {
  append_owned_points(in, order, true, pl);
  pl.n_pt = (int)pl.pt_user_of_int.size();
}

// ---- landmark-major observation list ----
// = the per-point lists in the final landmark order (key: landmark, pose, insertion).
// Per landmark: its observations and its (landmark, pose) pairs — one per distinct
// optimisable pose, carried by the LAST inserted observation of that pose (reference
// :826: B_ji is assigned, not accumulated).  Counts first, prefix sums, then every
// landmark fills its own ranges: parallel over landmarks.

// The pair rule, stated once: walking a landmark's slots in (pose, insertion) order, a slot
// of an optimisable pose opens a new pair when its pose differs from the previous slot's;
// otherwise it takes the pair id over from that slot, which loses it.
struct PairCursor {
  int64_t pw;         // id of the pair that is open (first pair of the landmark - 1 before any)
  int32_t last = -1;  // optimisable pose of the previous slot, -1: none
  // slot of pose ji (`opt`: landmark and pose optimisable): true when it opens a new pair
  bool opens(int32_t ji, bool opt) {
    const bool o = opt && ji != last;
    last = opt ? ji : -1;
    if (o) ++pw;
    return o;
  }
};

// one slot of the landmark-major list, without a pair id
void file_slot(Plan &pl, bool slim, int64_t s, int32_t pi, int32_t cam, int32_t ji, double u, double v) {
  pl.obs_idx[4 * s + 0] = cam;
  pl.obs_idx[4 * s + 1] = ji;
  pl.obs_idx[4 * s + 2] = pi;
  pl.obs_idx[4 * s + 3] = -1;
  if (slim) {
    pl.obs_cp[2 * s + 0] = cam | (ji << 16);
    pl.obs_cp[2 * s + 1] = pi;
  }
  pl.obs_uv[2 * s + 0] = u;
  pl.obs_uv[2 * s + 1] = v;
}

// the pair of slot s (an optimisable pose of an optimised landmark): true when it is a new one
bool assign_pair(Plan &pl, PairCursor &cur, int64_t s, int32_t pi, int32_t ji) {
  const bool opened = cur.opens(ji, true);
  if (opened) {
    pl.pair_pose[cur.pw] = ji;
    pl.pair_lm[cur.pw] = pi;
  } else {
    pl.obs_idx[4 * (s - 1) + 3] = -1;  // the earlier insertion loses its B_ji to this one (reference :826)
  }
  pl.obs_idx[4 * s + 3] = (int32_t)cur.pw;
  return opened;
}

// landmark-major ranges of every owned point: observation slots and pairs
struct LmRanges {
  std::vector<int64_t> optr, pptr;    // n_pt + 1
  std::vector<int32_t> group_of;      // M_grp: group of every grouped landmark
  // the masked group of landmark pi (masked groups pad their members to the union), or null
  const Plan::GrpRange *masked_group(const Plan &pl, int64_t pi) const {
    if (pi >= pl.M_grp) return nullptr;
    const Plan::GrpRange &gr = pl.grp_range[group_of[pi]];
    return gr.masked ? &gr : nullptr;
  }
};

// count pass: slots and pairs per landmark, then their prefix sums
LmRanges count_landmark_major(int threads, const PointObs &po, const Plan &pl) {
  LmRanges r;
  r.optr.assign((size_t)pl.n_pt + 1, 0);
  r.pptr.assign((size_t)pl.n_pt + 1, 0);
  r.group_of.assign((size_t)pl.M_grp, -1);
  for (size_t gidx = 0; gidx < pl.grp_range.size(); ++gidx)
    for (int l = pl.grp_range[gidx].l0; l < pl.grp_range[gidx].l0 + pl.grp_range[gidx].nl; ++l) r.group_of[l] = (int32_t)gidx;
  parallel_for(threads, pl.n_pt, [&](int64_t a0, int64_t a1) {
    for (int64_t pi = a0; pi < a1; ++pi) {
      const int q = pl.pt_user_of_int[pi];
      if (const Plan::GrpRange *gr = r.masked_group(pl, pi)) {
        r.optr[pi + 1] = gr->no;
        r.pptr[pi + 1] = gr->d;
        continue;
      }
      r.optr[pi + 1] = po.count(q);
      PairCursor cur{0};
      for (int64_t t = po.begin(q); t < po.end(q); ++t) cur.opens(po.rec[t].pose, pi < pl.M && po.rec[t].pose < pl.N);
      r.pptr[pi + 1] = cur.pw;
    }
  });
  for (int pi = 0; pi < pl.n_pt; ++pi) {
    r.optr[pi + 1] += r.optr[pi];
    r.pptr[pi + 1] += r.pptr[pi];
  }
  return r;
}

// a member of a masked group: the union's slots in order; this landmark's observations are
// a subsequence, the other slots are padded (uv = NaN), a pair without a valid slot is padded
void fill_masked_member(const PointObs &po, const Plan::GrpRange &gr, bool slim, int32_t pi, int64_t s, int64_t p0, Plan &pl) {
  const int q = pl.pt_user_of_int[pi];
  const double nan = std::numeric_limits<double>::quiet_NaN();
  int64_t t = po.begin(q);
  PairCursor cur{p0 - 1};
  bool pose_seen = false;
  for (int e = 0; e < gr.no; ++e, ++s) {
    const uint64_t w = pl.grp_upat[gr.upat0 + e];
    const int32_t ji = (int32_t)(w >> 32), cam = (int32_t)(uint32_t)w;
    const bool have = t < po.end(q) && po.rec[t].pose == ji && po.rec[t].cam == cam;
    file_slot(pl, slim, s, pi, cam, ji, have ? po.rec[t].u : nan, have ? po.rec[t].v : nan);
    if (ji < pl.N) {
      if (assign_pair(pl, cur, s, pi, ji)) pose_seen = false;
      pose_seen = pose_seen || have;
      pl.pair_pad[cur.pw] = pose_seen ? 0 : 1;
    } else {
      cur.opens(ji, false);
    }
    if (have) ++t;
  }
}

// every other landmark: its observations as they are
void fill_plain_landmark(const PointObs &po, bool slim, int32_t pi, int64_t s, int64_t p0, Plan &pl) {
  const int q = pl.pt_user_of_int[pi];
  PairCursor cur{p0 - 1};
  for (int64_t t = po.begin(q); t < po.end(q); ++t, ++s) {
    const ObsRecP &r = po.rec[t];
    file_slot(pl, slim, s, pi, r.cam, r.pose, r.u, r.v);
    if (pi < pl.M && r.pose < pl.N)
      assign_pair(pl, cur, s, pi, r.pose);
    else
      cur.opens(r.pose, false);
  }
}

std::string build_landmark_major(int threads, const PointObs &po, Plan &pl) {
  const int n_own = pl.n_pt, M = pl.M;
  const LmRanges r = count_landmark_major(threads, po, pl);
  pl.n_obs = r.optr[n_own];
  const int64_t P = r.pptr[n_own];
  if (P >= (int64_t)INT32_MAX) return "too many pairs for int32 pair ids";
  pl.obs_idx.resize((size_t)pl.n_obs * 4);
  pl.obs_uv.resize((size_t)pl.n_obs * 2);
  const bool slim = pl.n_cam < 65536 && pl.n_pose < 65536;
  if (slim) pl.obs_cp.resize((size_t)pl.n_obs * 2);
  pl.pair_pose.resize((size_t)P);
  pl.pair_lm.resize((size_t)P);
  pl.pair_pad.assign((size_t)P, 0);
  parallel_for(threads, n_own, [&](int64_t a0, int64_t a1) {
    for (int64_t pi = a0; pi < a1; ++pi) {
      if (const Plan::GrpRange *gr = r.masked_group(pl, pi))
        fill_masked_member(po, *gr, slim, (int32_t)pi, r.optr[pi], r.pptr[pi], pl);
      else
        fill_plain_landmark(po, slim, (int32_t)pi, r.optr[pi], r.pptr[pi], pl);
    }
  });
  // (the optimised landmarks come first: their ranges are the lists' prefixes)
  pl.lm_obs_ptr.assign(r.optr.begin(), r.optr.begin() + M + 1);
  pl.lm_pair_ptr.assign(r.pptr.begin(), r.pptr.begin() + M + 1);
  pl.n_pair_pad = 0;
  for (uint8_t v : pl.pair_pad) pl.n_pair_pad += v;
  pl.n_obs_opt = pl.lm_obs_ptr[M];
  pl.P = P;
  return std::string();
}

// ---- pose-major observation list (optimisable poses) ----
void build_pose_major(Plan &pl) {
  const int N = pl.N;
  std::vector<int64_t> psel;
  // (the landmark-major list is in landmark order: the grouped landmarks' observations,
  //  which never enter, are its first lm_obs_ptr[M_grp] entries)
  const int64_t s_first = pl.lin_groups ? pl.lm_obs_ptr[pl.M_grp] : 0;
  psel.reserve((size_t)(pl.n_obs - s_first));
  // (observations of landmarks in covisibility groups are linearised, pose side
  //  included, by k_lin_grp: they do not enter the pose-major list)
  for (int64_t s = s_first; s < pl.n_obs; ++s)
    if (pl.obs_idx[4 * s + 1] < N && !(pl.lin_groups && pl.obs_idx[4 * s + 2] < pl.M_grp)) psel.push_back(s);
  // stable counting sort by pose keeps (point, insertion) order inside
  pl.pose_obs_ptr.assign(N + 1, 0);
  for (int64_t s : psel) pl.pose_obs_ptr[pl.obs_idx[4 * s + 1] + 1]++;
  for (int j = 0; j < N; ++j) pl.pose_obs_ptr[j + 1] += pl.pose_obs_ptr[j];
  pl.n_pobs = (int64_t)psel.size();
  pl.pobs_idx.resize((size_t)pl.n_pobs * 2);
  pl.pobs_uv.resize((size_t)pl.n_pobs * 2);
  std::vector<int64_t> cur(pl.pose_obs_ptr.begin(), pl.pose_obs_ptr.end() - 1);
  for (int64_t s : psel) {
    const int j = pl.obs_idx[4 * s + 1];
    const int64_t d = cur[j]++;
    pl.pobs_idx[2 * d + 0] = pl.obs_idx[4 * s + 0];  // camera
    pl.pobs_idx[2 * d + 1] = pl.obs_idx[4 * s + 2];  // point (the pose is the list's own)
    pl.pobs_uv[2 * d + 0] = pl.obs_uv[2 * s + 0];
    pl.pobs_uv[2 * d + 1] = pl.obs_uv[2 * s + 1];
  }
  // one wave per chunk: aim at ~kPoseWaveTarget waves in total (one resident
  // round on the GPU), each pose's list split into equal chunks
  int64_t cap = (pl.n_pobs + kPoseWaveTarget - 1) / kPoseWaveTarget;
  cap = (cap + 63) / 64 * 64;
  cap = std::min<int64_t>(std::max<int64_t>(cap, kPoseChunkMin), kPoseChunkMax);
  make_chunks(pl.pose_obs_ptr, N, (int)cap, pl.achunk_pose, pl.achunk_begin, pl.achunk_end, pl.pose_achunk_ptr);
}

// ---- Schur complement structure ----
// Non-zero upper blocks (j <= k) of S = union over landmarks of J(i) x J(i),
// plus every diagonal.  Landmarks are processed LANDMARK-MAJOR by "Schur
// workgroups": a workgroup stages the W blocks of a run of consecutive
// landmarks (<= kSchurPairs pairs) in LDS and accumulates their
// contributions into workgroup-local block SLOTS; a second kernel sums the
// slots of each block in workgroup order (deterministic).  Landmarks seen by
// more than kSchurPairs poses go through the global (j,k)-sorted triple list.

using BlockRows = std::vector<std::vector<int32_t>>;  // per pose row j: columns k >= j, unsorted, with repeats

void sort_rows(BlockRows &rowk) {
  for (auto &rk : rowk) {
    std::sort(rk.begin(), rk.end());
    rk.erase(std::unique(rk.begin(), rk.end()), rk.end());
  }
}
// J x J of a run of ascending poses; skip_repeats: not behind the same column again
template <class PoseAt>
void add_pose_set(BlockRows &rowk, int64_t b, int64_t e, bool skip_repeats, const PoseAt &pose_at) {
  for (int64_t p = b; p < e; ++p) {
    auto &rk = rowk[pose_at(p)];
    for (int64_t q = p; q < e; ++q) {
      const int32_t k = pose_at(q);
      if (!skip_repeats || rk.empty() || rk.back() != k) rk.push_back(k);
    }
  }
}
// one shard: the pair lists hold every optimised landmark
void blocks_from_pairs(const Plan &pl, BlockRows &rowk) {
  const auto pose_at = [&pl](int64_t p) { return pl.pair_pose[p]; };
  // (the landmarks of a covisibility group share one pose set: its first landmark
  //  stands for all of them)
  for (const Plan::GrpRange &gr : pl.grp_range) add_pose_set(rowk, pl.lm_pair_ptr[gr.l0], pl.lm_pair_ptr[gr.l0 + 1], false, pose_at);
  for (int i = pl.M_grp; i < pl.M; ++i) add_pose_set(rowk, pl.lm_pair_ptr[i], pl.lm_pair_ptr[i + 1], true, pose_at);
}
// several shards: the block set is the GLOBAL one (all shards use the same block numbering:
// the packed S||rhs exchange buffer is indexed by block), from the full observation list
void blocks_from_observations(const PlanInput &in, const Plan &pl, BlockRows &rowk) {
  std::vector<uint64_t> keys;
  keys.reserve(in.n_obs);
  for (int64_t k = 0; k < in.n_obs; ++k) {
    const int j = pl.pose_int_of_user[in.obs_pose[k]];
    if (j < pl.N && !in.pt_fixed[in.obs_pt[k]]) keys.push_back(((uint64_t)(uint32_t)in.obs_pt[k] << 32) | (uint32_t)j);
  }
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  const auto pose_at = [&keys](int64_t u) { return (int32_t)(uint32_t)keys[u]; };
  size_t a = 0;
  while (a < keys.size()) {
    size_t b = a;
    while (b < keys.size() && (keys[b] >> 32) == (keys[a] >> 32)) ++b;
    add_pose_set(rowk, (int64_t)a, (int64_t)b, true, pose_at);
    a = b;
  }
}
// relative-pose factors (PlanInput::rel_j / rel_k): every pair of two optimisable
// poses is an upper block too, added once when covisibility did not produce it —
// such a block has no slot contribution and no triple.  Returns their number.
int64_t blocks_from_factors(const PlanInput &in, const Plan &pl, BlockRows &rowk) {
  std::vector<uint64_t> rel_new;  // (j << 32 | k) of the blocks that only a factor asks for
  sort_rows(rowk);
  for (int64_t f = 0; f < in.n_rel; ++f) {
    const int32_t a = pl.pose_int_of_user[in.rel_j[f]], b = pl.pose_int_of_user[in.rel_k[f]];
    if (a >= pl.N || b >= pl.N) continue;
    const int32_t j = std::min(a, b), k = std::max(a, b);
    if (!std::binary_search(rowk[j].begin(), rowk[j].end(), k)) rel_new.push_back(((uint64_t)(uint32_t)j << 32) | (uint32_t)k);
  }
  std::sort(rel_new.begin(), rel_new.end());
  rel_new.erase(std::unique(rel_new.begin(), rel_new.end()), rel_new.end());
  for (uint64_t key : rel_new) rowk[(int)(key >> 32)].push_back((int32_t)(uint32_t)key);
  return (int64_t)rel_new.size();
}

// The block set as a CSR over pose rows: block ids of row j are [row_ptr[j], row_ptr[j + 1]),
// columns ascending in Plan::sblk_k, (j, j) first.
struct BlockIndex {
  std::vector<int64_t> row_ptr;  // N + 1
  const std::vector<int32_t> *sblk_k = nullptr;
  int32_t block_of(int32_t j, int32_t k) const {
    const int32_t *b0 = sblk_k->data() + row_ptr[j], *e0 = sblk_k->data() + row_ptr[j + 1];
    return (int32_t)(std::lower_bound(b0, e0, k) - sblk_k->data());
  }
};

// Fills sblk_j / sblk_k, B, diag_blk, n_rel, n_rel_only.
BlockIndex build_block_set(const PlanInput &in, Plan &pl) {
  const int N = pl.N;
  BlockRows rowk(N);
  for (int j = 0; j < N; ++j) rowk[j].push_back(j);
  if (in.world == 1)
    blocks_from_pairs(pl, rowk);
  else
    blocks_from_observations(in, pl, rowk);
  pl.n_rel = in.n_rel;
  pl.n_rel_only = in.n_rel > 0 ? blocks_from_factors(in, pl, rowk) : 0;
  sort_rows(rowk);
  BlockIndex bi;
  bi.row_ptr.assign((size_t)N + 1, 0);
  for (int j = 0; j < N; ++j) {
    for (int32_t k : rowk[j]) {
      pl.sblk_j.push_back(j);
      pl.sblk_k.push_back(k);
    }
    bi.row_ptr[j + 1] = (int64_t)pl.sblk_j.size();
  }
  pl.B = (int64_t)pl.sblk_j.size();
  pl.diag_blk.resize(N);
  for (int j = 0; j < N; ++j) pl.diag_blk[j] = (int32_t)bi.row_ptr[j];  // (j,j) leads row j
  bi.sblk_k = &pl.sblk_k;
  return bi;
}

// the factors of every optimisable pose and of every coupled block, in input order
// (rel_jk, rel_pptr / rel_plist, rel_blk / rel_bptr / rel_blist; all empty without factors)
void build_relative_lists(const PlanInput &in, const BlockIndex &blocks, Plan &pl) {
  if (in.n_rel <= 0) return;
  // the factors name internal poses here (the optimisable ones come first); a coupled block's
  // key is its id in sblk_j / sblk_k, where S_jk of a factor with j > k lies transposed
  const int N = pl.N;
  std::vector<int32_t> j((size_t)in.n_rel), k((size_t)in.n_rel), opt_of((size_t)in.n_pose, -1);
  for (int64_t f = 0; f < in.n_rel; ++f) {
    j[f] = pl.pose_int_of_user[in.rel_j[f]];
    k[f] = pl.pose_int_of_user[in.rel_k[f]];
  }
  std::iota(opt_of.begin(), opt_of.begin() + N, 0);
  RelLists l;
  relative_build_lists(
      in.n_rel, j.data(), k.data(), N, opt_of.data(),
      [&](int32_t a, int32_t b) {
        return std::pair<int64_t, bool>(blocks.block_of(std::min(a, b), std::max(a, b)), a > b);
      },
      &l);
  pl.rel_jk.swap(l.jk);
  pl.rel_pptr.swap(l.pptr);
  pl.rel_plist.swap(l.plist);
  pl.rel_blk.assign(l.bkey.begin(), l.bkey.end());
  pl.rel_bptr.swap(l.bptr);
  pl.rel_blist.swap(l.blist);
}

// Landmark kinds: 0 = fits a super-run whole; 1 = SPLIT: its pairs fit the LDS
// staging (<= kSchurPairs) but its d (d + 1) / 2 blocks exceed the kSchurSlots
// register slots of a run: the pose list is cut into g groups of <= kSplit
// poses and the landmark is processed once per CLASS (a, b), a <= b < g — the
// triples (p, q) with p in group a and q in group b: at most kSplit^2 <= 128
// blocks — in a separate run; 2 = big (more pairs than the staging holds, or
// PlanKnobs::split off): global triple list.
constexpr int kSplit = 11;
static_assert(kSplit * kSplit <= kSchurSlots && kSplit * kSplit <= kSchurTri, "class size");
struct LandmarkKinds {
  const Plan &pl;
  const bool split;
  int64_t degree(int l) const { return pl.lm_pair_ptr[l + 1] - pl.lm_pair_ptr[l]; }
  // does not fit a super-run whole ...
  static bool is_big(int64_t d) { return d * (d + 1) / 2 > kSchurTri || d * (d + 1) / 2 > kSchurSlots || d > kSchurPairs; }
  // ... and cannot be split into classes either (its pairs exceed the LDS staging): global list
  bool is_list(int64_t d) const { return is_big(d) && (d > kSchurPairs || !split); }
  int kind_of(int l) const { return !is_big(degree(l)) ? 0 : is_list(degree(l)) ? 2 : 1; }
  int pose_groups(int l) const { return (int)((degree(l) + kSplit - 1) / kSplit); }
};
// One class (ca, cb) of pose groups of `sp` poses; sp == 0: the whole landmark.
struct PoseClass {
  int sp, ca, cb;
  // triples of a landmark with d pairs in this class
  int64_t triples(int64_t d) const {
    if (sp == 0) return d * (d + 1) / 2;
    const int64_t na = std::min<int64_t>(sp, d - (int64_t)ca * sp), nb = std::min<int64_t>(sp, d - (int64_t)cb * sp);
    if (na <= 0 || nb <= 0) return 0;
    return ca == cb ? na * (na + 1) / 2 : na * nb;
  }
  // the triple of the landmark's lp-th and lq-th pair
  bool holds(int64_t lp, int64_t lq) const { return sp == 0 || (lp / sp == ca && lq / sp == cb); }
};

// (a) big landmarks -> global triple list sorted by (block, landmark): T, tri_p / tri_q,
// sblk_tri_ptr, the tchunk arrays.  Returns the triples that are NOT on the list.
int64_t build_big_triple_list(const LandmarkKinds &kinds, const BlockIndex &blocks, Plan &pl) {
  int64_t Tbig = 0, Tall = 0;
  for (int i = 0; i < pl.M; ++i) {
    const int64_t d = kinds.degree(i);
    Tall += d * (d + 1) / 2;
    if (i >= pl.M_grp && kinds.is_list(d)) Tbig += d * (d + 1) / 2;  // (grouped landmarks: k_schur_grp's)
  }
  pl.T = Tall;
  std::vector<std::pair<int32_t, std::pair<int64_t, int64_t>>> big;
  big.reserve(Tbig);
  for (int i = pl.M_grp; i < pl.M; ++i) {
    const int64_t p0 = pl.lm_pair_ptr[i], p1 = pl.lm_pair_ptr[i + 1];
    if (!kinds.is_list(p1 - p0)) continue;
    for (int64_t p = p0; p < p1; ++p)
      for (int64_t q = p; q < p1; ++q) big.push_back({blocks.block_of(pl.pair_pose[p], pl.pair_pose[q]), {p, q}});
  }
  std::stable_sort(big.begin(), big.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
  pl.tri_p.resize(big.size());
  pl.tri_q.resize(big.size());
  pl.sblk_tri_ptr.assign(pl.B + 1, 0);
  for (size_t t = 0; t < big.size(); ++t) {
    pl.tri_p[t] = big[t].second.first;
    pl.tri_q[t] = big[t].second.second;
    pl.sblk_tri_ptr[big[t].first + 1]++;
  }
  for (int64_t bk = 0; bk < pl.B; ++bk) pl.sblk_tri_ptr[bk + 1] += pl.sblk_tri_ptr[bk];
  make_chunks(pl.sblk_tri_ptr, (int)pl.B, kTriChunk, pl.tchunk_blk, pl.tchunk_begin, pl.tchunk_end, pl.sblk_tchunk_ptr);
  return Tall - Tbig;
}

using Contrib = std::vector<std::pair<int32_t, int32_t>>;  // (block, flat slot), ascending slot

// (a') covisibility groups, group by group: its pattern (grp_pat), its k_lin_grp pieces
// (lin_desc, n_apart2) and its k_schur_grp pieces (grp32 / grp64 / grp128) with their slots.

// observation pattern of the group, from its first landmark; returns its first entry
// or -1 when the pose count does not match
int32_t append_group_pattern(const Plan::GrpRange &gr, Plan &pl) {
  const int32_t pat0 = (int32_t)(pl.grp_pat.size() / 2);
  const int64_t ob = pl.lm_obs_ptr[gr.l0];
  int jj = -1;
  int32_t lastp = -1;
  for (int oo = 0; oo < gr.no; ++oo) {
    const int32_t ji = pl.obs_idx[4 * (ob + oo) + 1], cam = pl.obs_idx[4 * (ob + oo) + 0];
    const bool opt = ji < pl.N;
    if (opt && ji != lastp) ++jj;
    lastp = ji;
    const bool lastw = pl.obs_idx[4 * (ob + oo) + 3] >= 0;
    pl.grp_pat.push_back(ji);
    pl.grp_pat.push_back(cam | ((opt ? jj : 0) << 16) | (opt ? 1 << 29 : 0) | (lastw ? 1 << 30 : 0));
  }
  return jj + 1 == gr.d ? pat0 : -1;
}
// k_lin_grp pieces: runs of `steps` wave steps (4 waves x nlw landmarks each), the
// pieces of a group equal up to one step
void append_lin_pieces(const Plan::GrpRange &gr, int steps, int32_t pat0, Plan &pl) {
  const int64_t p0 = pl.lm_pair_ptr[gr.l0];
  const int per_step = 4 * lin_grp_nlw(gr.no);
  const int nstep = (gr.nl + per_step - 1) / per_step;
  const int npiece = (nstep + steps - 1) / steps;
  for (int c = 0; c < npiece; ++c) {
    const int s0 = (int)((int64_t)nstep * c / npiece), s1 = (int)((int64_t)nstep * (c + 1) / npiece);
    Plan::LinDesc ld;
    const int il0 = s0 * per_step, il1 = std::min(gr.nl, s1 * per_step);
    ld.l0 = gr.l0 + il0;
    ld.nl = il1 - il0;
    ld.d = gr.d;
    ld.no = gr.no;
    ld.p0 = p0 + (int64_t)gr.d * il0;
    ld.o0 = pl.lm_obs_ptr[ld.l0];
    ld.pat0 = pat0;
    ld.apart0 = (int32_t)pl.n_apart2;
    ld.cost_idx = 0;  // set by finish_lin_grp_bookkeeping, after the chunks are known
    ld.pad_ = gr.masked;  // 1: padded slots (uv = NaN) and a dynamic last writer
    pl.n_apart2 += gr.d;
    if (ld.nl > 0) pl.lin_desc.push_back(ld);
  }
}
// one k_schur_grp workgroup per (piece of a) group, d (d + 1) / 2 slots each, in (jj, kk)
// row-major order of the upper triangle
void append_schur_pieces(const Plan::GrpRange &gr, const BlockIndex &blocks, Contrib &contrib, Plan &pl) {
  const int64_t p0 = pl.lm_pair_ptr[gr.l0];
  // (wide groups, d > 10: k_schur_grp_wide is bound by the fp64 matrix pipe — 27 MFMAs per
  //  landmark — and a 20-pose window of a few hundred landmarks is one long workgroup:
  //  pieces of <= kGrpWidePiece landmarks spread them over the CUs)
  const int cap = gr.d > 10 ? kGrpWidePiece : kGrpMaxLandmarks;
  const int pieces = (gr.nl + cap - 1) / cap;
  const int per = (gr.nl + pieces - 1) / pieces;
  for (int c0 = 0; c0 < gr.nl; c0 += per) {
    Plan::GrpDesc gd = Plan::GrpDesc();
    gd.l0 = gr.l0 + c0;
    gd.nl = std::min(per, gr.nl - c0);
    gd.d = gr.d;
    gd.p0 = p0 + (int64_t)gr.d * c0;
    gd.s0 = (int32_t)pl.slot_blk.size();
    for (int t = 0; t < kGrpMaxPoses; ++t) gd.pose[t] = t < gr.d ? pl.pair_pose[p0 + t] : 0;
    for (int jj = 0; jj < gr.d; ++jj)
      for (int kk = jj; kk < gr.d; ++kk) {
        const int32_t bk = blocks.block_of(gd.pose[jj], gd.pose[kk]);
        contrib.push_back({bk, (int32_t)pl.slot_blk.size()});
        pl.slot_blk.push_back(bk);
      }
    (gr.d <= 5 ? pl.grp32 : gr.d <= 10 ? pl.grp64 : pl.grp128).push_back(gd);
  }
}
std::string build_group_pieces(const PlanKnobs &knobs, const BlockIndex &blocks, Contrib &contrib, Plan &pl) {
  const int steps = knobs.lin_steps > 0 ? knobs.lin_steps : kLinGrpSteps;
  for (const Plan::GrpRange &gr : pl.grp_range) {
    for (int l = gr.l0; l < gr.l0 + gr.nl; ++l)
      if (pl.lm_pair_ptr[l + 1] - pl.lm_pair_ptr[l] != gr.d || pl.lm_obs_ptr[l + 1] - pl.lm_obs_ptr[l] != gr.no)
        return "internal: covisibility group with a ragged landmark";
    const int32_t pat0 = append_group_pattern(gr, pl);
    if (pat0 < 0) return "internal: covisibility group pattern / pose count mismatch";
    append_lin_pieces(gr, steps, pat0, pl);
    // (d == 0: no pair, no Schur contribution: no k_schur_grp workgroup)
    if (gr.d > 0) append_schur_pieces(gr, blocks, contrib, pl);
  }
  return std::string();
}

// (b) SUPER-RUNS over the remaining landmarks: maximal runs of consecutive
// landmarks (locality order) that touch at most kSchurSlots distinct
// blocks; one workgroup per super-run keeps one 6x6 accumulator per
// (slot, lane) in registers while it streams the run's W blocks through
// LDS in CHUNKS (<= kSchurPairs pairs, <= kSchurTri triples).
// Fills sup_desc, sup_lane, chunk_desc, chunk_sp, ltri and appends to slot_blk.
struct RunBuilder {
  Plan &pl;
  const BlockIndex &blocks;
  const int sup_cap;   // landmarks per run
  const bool stats;    // PlanKnobs::stats
  Contrib contrib;                                // of the group pieces and the runs
  std::vector<int32_t> mark;                      // block -> local slot of the current run, -1 outside
  std::vector<int32_t> sup_blocks;                // blocks of the current run, in order of appearance
  std::vector<std::pair<int32_t, uint32_t>> loc;  // (slot, triple word) of the current chunk
  std::vector<int64_t> tcount;                    // triples per slot of the current run
  double sum_max = 0, sum_ideal = 0, sum_mean_active = 0;  // balance of the triple loop over n_ch chunks
  long n_ch = 0;
  std::string error;

  RunBuilder(Plan &pl_, const BlockIndex &blocks_, int sup_cap_, bool stats_)
      : pl(pl_), blocks(blocks_), sup_cap(sup_cap_), stats(stats_), mark((size_t)pl_.B, -1) {}

  // The greedy chunk-cut rule, stated once: a chunk that holds landmarks already takes no
  // further one with dd pairs and dt triples when a staging limit would be exceeded.
  struct ChunkFill {
    int nl = 0;
    int64_t np = 0, nt = 0;
    void add(int64_t dd, int64_t dt) { ++nl, np += dd, nt += dt; }
  };
  static bool chunk_would_overflow(const ChunkFill &c, int64_t dd, int64_t dt) {
    return c.nl > 0 && (c.np + dd > kSchurPairs || c.nt + dt > kSchurTri || c.nl >= kSchurLandmarks);
  }
  int64_t degree(int l) const { return pl.lm_pair_ptr[l + 1] - pl.lm_pair_ptr[l]; }
  void unmark() {
    for (int32_t bk : sup_blocks) mark[bk] = -1;
  }

  // Grows a run from landmark i0: until sup_cap landmarks, kSchurSuperChunks chunks or
  // kSchurSlots blocks are reached (the first landmark is always taken).  Leaves the run's
  // blocks in sup_blocks / mark and returns the end of the run.
  int grow_run(int i0, int hi, const PoseClass &cls) {
    sup_blocks.clear();
    int i = i0, nchunk = 1;
    ChunkFill fill;  // the run's last chunk so far
    while (i < hi && i - i0 < sup_cap) {
      const int64_t p0 = pl.lm_pair_ptr[i], p1 = pl.lm_pair_ptr[i + 1];
      if (chunk_would_overflow(fill, p1 - p0, cls.triples(p1 - p0))) {
        if (nchunk == kSchurSuperChunks) break;  // descriptor table in LDS is full
        ++nchunk;
        fill = ChunkFill();
      }
      fill.add(p1 - p0, cls.triples(p1 - p0));
      // blocks this landmark would add
      const size_t before = sup_blocks.size();
      for (int64_t p = p0; p < p1; ++p)
        for (int64_t q = p; q < p1; ++q) {
          if (!cls.holds(p - p0, q - p0)) continue;
          const int32_t bk = blocks.block_of(pl.pair_pose[p], pl.pair_pose[q]);
          if (mark[bk] < 0) {
            mark[bk] = (int32_t)sup_blocks.size();
            sup_blocks.push_back(bk);
          }
        }
      if ((int)sup_blocks.size() > kSchurSlots && i > i0) {
        for (size_t s2 = before; s2 < sup_blocks.size(); ++s2) mark[sup_blocks[s2]] = -1;
        sup_blocks.resize(before);
        break;
      }
      ++i;
    }
    return i;
  }

  // one chunk of landmarks [c0, l) with np pairs: its triples sorted by slot (mark), its
  // per-slot offsets and its descriptor; nothing when it has no triple of the class
  void emit_chunk(int c0, int l, int64_t np, int ns, const PoseClass &cls) {
    const int64_t pbase = pl.lm_pair_ptr[c0];
    loc.clear();
    for (int m = c0; m < l; ++m) {
      const int64_t q0 = pl.lm_pair_ptr[m];
      for (int64_t p = q0; p < pl.lm_pair_ptr[m + 1]; ++p)
        for (int64_t q = p; q < pl.lm_pair_ptr[m + 1]; ++q)
          if (cls.holds(p - q0, q - q0))
            loc.push_back({mark[blocks.block_of(pl.pair_pose[p], pl.pair_pose[q])],
                           (uint32_t)(((p - pbase) << 16) | ((uint32_t)(m - c0) << 8) | (q - pbase))});
    }
    if (loc.empty()) return;  // (landmarks without pairs)
    std::stable_sort(loc.begin(), loc.end(), [](const auto &x, const auto &y) { return x.first < y.first; });
    Plan::ChunkDesc cd;
    cd.p0 = pbase;
    while (pl.ltri.size() & 3) pl.ltri.push_back(0u);  // chunks start 16-byte aligned
    cd.tb = (int64_t)pl.ltri.size();
    cd.sp = (int64_t)pl.chunk_sp.size();
    cd.l0 = c0;
    cd.nl = l - c0;
    cd.np = (int32_t)np;
    cd.nt = (int32_t)loc.size();
    // per-slot offsets into this chunk's triple list
    size_t t = 0;
    for (int s2 = 0; s2 <= ns; ++s2) {
      while (t < loc.size() && loc[t].first < s2) ++t;
      pl.chunk_sp.push_back((uint16_t)t);
    }
    for (auto &e : loc) {
      pl.ltri.push_back(e.second);
      tcount[e.first]++;
    }
    pl.chunk_desc.push_back(cd);
  }

  // the run [i0, i1) cut into chunks by the greedy rule
  void cut_chunks(int i0, int i1, int ns, const PoseClass &cls) {
    tcount.assign(ns, 0);
    int l = i0;
    while (l < i1) {
      const int c0 = l;
      ChunkFill fill;
      while (l < i1 && !chunk_would_overflow(fill, degree(l), cls.triples(degree(l)))) {
        fill.add(degree(l), cls.triples(degree(l)));
        ++l;
      }
      emit_chunk(c0, l, fill.np, ns, cls);
    }
  }

  // balance of the triple loop of run sd (developer knob)
  void add_stats(const Plan::SupDesc &sd) {
    const uint32_t *lw = &pl.sup_lane[pl.sup_lane.size() - 256];
    std::vector<int> tps2(sd.ns, 1);
    for (int q = 0; q < 256; ++q)
      if ((lw[q] & 0xffu) < (uint32_t)sd.ns) tps2[lw[q] & 0xffu] = (lw[q] >> 14) & 0x3f;
    for (int c = sd.chunk_begin; c < sd.chunk_end; ++c) {
      const uint16_t *sp2 = &pl.chunk_sp[pl.chunk_desc[c].sp];
      int mx = 0, tot = 0, act = 0;
      for (int q = 0; q < sd.ns; ++q) {
        const int cnt2 = sp2[q + 1] - sp2[q];
        tot += cnt2;
        act += cnt2 > 0;
        mx = std::max(mx, (cnt2 + tps2[q] - 1) / tps2[q]);
      }
      sum_max += mx;
      sum_ideal += tot * 2.0 / 256.0;
      sum_mean_active += act;
      ++n_ch;
    }
  }
  void print_stats() const {
    if (n_ch > 0)
      fprintf(stderr, "[plan] chunks %ld: triple-loop iterations per chunk: busiest lane %.2f, ideal %.2f; "
                      "active slots %.1f\n",
              n_ch, sum_max / n_ch, sum_ideal / n_ch, sum_mean_active / n_ch);
  }

  // the run [i0, i1) whose blocks grow_run left in sup_blocks: slots, chunks, lane table
  void emit_run(int i0, int i1, const PoseClass &cls) {
    const int ns = (int)sup_blocks.size();
    if (ns > kSchurSlots) {
      error = "internal: landmark class exceeds kSchurSlots blocks";
      return;
    }
    // slots sorted by block id for a stable order
    std::vector<int32_t> order(sup_blocks);
    std::sort(order.begin(), order.end());
    for (int s2 = 0; s2 < ns; ++s2) mark[order[s2]] = s2;
    Plan::SupDesc sd;
    sd.s0 = (int32_t)pl.slot_blk.size();
    sd.ns = ns;
    sd.chunk_begin = (int32_t)pl.chunk_desc.size();
    for (int s2 = 0; s2 < ns; ++s2) {
      contrib.push_back({order[s2], sd.s0 + s2});
      pl.slot_blk.push_back(order[s2]);
    }
    cut_chunks(i0, i1, ns, cls);
    sd.chunk_end = (int32_t)pl.chunk_desc.size();
    if (sd.chunk_end - sd.chunk_begin > kSchurSuperChunks) {
      error = "internal: super-run exceeds kSchurSuperChunks chunks";
      return;
    }
    if (sd.chunk_end == sd.chunk_begin) {  // nothing to do after all: drop the run's slots
      contrib.resize(contrib.size() - ns);
      pl.slot_blk.resize(pl.slot_blk.size() - ns);
      return;
    }
    pl.sup_desc.push_back(sd);
    deal_lanes(tcount, pl.sup_lane);
    if (stats) add_stats(sd);
  }

  // super-runs over the landmarks [lo, hi) (all of one kind), restricted to one class
  void build_runs(int lo, int hi, const PoseClass &cls) {
    int i = lo;
    while (i < hi && error.empty()) {
      const int i0 = i;
      i = grow_run(i0, hi, cls);
      if (sup_blocks.empty()) continue;  // landmarks without pairs
      emit_run(i0, i, cls);
      unmark();
    }
  }
};

// Maximal stretches of ungrouped landmarks of one kind (and, for split landmarks, one
// pose-group count) go to the run builder: whole, or once per class.
std::string build_super_runs(const LandmarkKinds &kinds, RunBuilder &runs, Plan &pl) {
  int i = pl.M_grp;
  while (i < pl.M && runs.error.empty()) {
    const int kd = kinds.kind_of(i);
    if (kd == 2) {  // handled by the global triple list
      ++i;
      continue;
    }
    int j = i + 1;
    while (j < pl.M && kinds.kind_of(j) == kd && (kd == 0 || kinds.pose_groups(j) == kinds.pose_groups(i))) ++j;
    if (kd == 0) {
      runs.build_runs(i, j, PoseClass{0, 0, 0});
    } else {
      const int g = kinds.pose_groups(i);
      for (int ca = 0; ca < g; ++ca)
        for (int cb = ca; cb < g; ++cb) runs.build_runs(i, j, PoseClass{kSplit, ca, cb});
    }
    i = j;
  }
  if (!runs.error.empty()) return runs.error;
  runs.print_stats();
  for (int k = 0; k < 4; ++k) pl.ltri.push_back(0u);  // the last chunk's 16-byte loads stay inside
  return std::string();
}

// per-block contribution lists (ascending super-run = ascending slot id)
void build_contrib_lists(const Contrib &contrib, Plan &pl) {
  pl.blk_contrib_ptr.assign(pl.B + 1, 0);
  for (auto &c2 : contrib) pl.blk_contrib_ptr[c2.first + 1]++;
  for (int64_t bk = 0; bk < pl.B; ++bk) pl.blk_contrib_ptr[bk + 1] += pl.blk_contrib_ptr[bk];
  pl.contrib_slot.resize(contrib.size());
  std::vector<int64_t> cur(pl.blk_contrib_ptr.begin(), pl.blk_contrib_ptr.end() - 1);
  for (auto &c2 : contrib) pl.contrib_slot[cur[c2.first]++] = c2.second;
}

std::string build_schur_structure(const PlanInput &in, const PlanKnobs &knobs, Plan &pl) {
  const BlockIndex blocks = build_block_set(in, pl);
  build_relative_lists(in, blocks, pl);
  const LandmarkKinds kinds{pl, knobs.split};
  const int64_t run_triples = build_big_triple_list(kinds, blocks, pl);
  pl.ltri.reserve((size_t)run_triples);
  RunBuilder runs(pl, blocks, schur_run_cap(pl.M - pl.M_grp, knobs.sup_cap), knobs.stats);
  std::string err = build_group_pieces(knobs, blocks, runs.contrib, pl);
  if (err.empty()) err = build_super_runs(kinds, runs, pl);
  if (err.empty()) build_contrib_lists(runs.contrib, pl);
  return err;
}

// ---- back-substitution chunks: consecutive landmarks, <= kSchurPairs pairs
// (a landmark with more pairs forms a chunk of its own) ----
void build_backsub_chunks(Plan &pl) {
  // (a chunk does not straddle M_grp: with lin_groups k_lin_landmarks starts
  //  at chunk n_bchunk_grp, the grouped landmarks are k_lin_grp's)
  pl.bchunk_lm.assign(1, 0);
  pl.n_bchunk_grp = 0;
  int l = 0;
  while (l < pl.M) {
    int64_t np = 0;
    const int c0 = l;
    const int lim = l < pl.M_grp ? pl.M_grp : pl.M;
    while (l < lim && l - c0 < kSchurLandmarks) {
      const int64_t dd = pl.lm_pair_ptr[l + 1] - pl.lm_pair_ptr[l];
      if (l > c0 && np + dd > kSchurPairs) break;
      np += dd;
      ++l;
    }
    pl.bchunk_lm.push_back(l);
    if (l <= pl.M_grp) pl.n_bchunk_grp = (int)pl.bchunk_lm.size() - 1;
  }
}

// ---- k_lin_grp bookkeeping: cost-partial entry of each group piece (after the
// chunks' entries), rows of Apart2 per pose ----
void finish_lin_grp_bookkeeping(Plan &pl) {
  const int N = pl.N;
  // plain pieces first, masked pieces behind them: one launch of each k_lin_grp form
  std::stable_partition(pl.lin_desc.begin(), pl.lin_desc.end(), [](const Plan::LinDesc &g) { return g.pad_ == 0; });
  pl.n_lin_plain = 0;
  for (auto &g : pl.lin_desc) pl.n_lin_plain += g.pad_ == 0;
  int32_t ci = (int32_t)pl.bchunk_lm.size() - 1;
  for (auto &g : pl.lin_desc) g.cost_idx = ci++;
  pl.pose_gpart_ptr.assign(N + 1, 0);
  if (!pl.lin_groups) {
    pl.n_apart2 = 0;
    pl.lin_desc.clear();
    pl.n_lin_plain = 0;
  }
  for (auto &g : pl.lin_desc)
    for (int t = 0; t < g.d; ++t) pl.pose_gpart_ptr[pl.pair_pose[g.p0 + t] + 1]++;
  for (int j = 0; j < N; ++j) pl.pose_gpart_ptr[j + 1] += pl.pose_gpart_ptr[j];
  pl.pose_gpart.assign((size_t)pl.pose_gpart_ptr[N], 0);
  std::vector<int32_t> cur(pl.pose_gpart_ptr.begin(), pl.pose_gpart_ptr.end() - 1);
  for (auto &g : pl.lin_desc)
    for (int t = 0; t < g.d; ++t) pl.pose_gpart[cur[pl.pair_pose[g.p0 + t]]++] = g.apart0 + t;
}

}  // namespace

std::string build_plan(const PlanInput &in, const PlanKnobs &knobs, Plan &pl) {
  std::string err = check_sizes(in);
  if (!err.empty()) return err;
  PhaseClock clk{knobs.times};
  const int threads = plan_threads(knobs.threads);
  err = validate_observations(in, threads);
  if (!err.empty()) return err;
  pl = Plan();
  pl.n_cam = in.n_cam;
  pl.n_pose = in.n_pose;
  pl.n_pt_global = in.n_pt;
  pl.n_obs_global = in.n_obs;
  order_poses(in, pl.pose_int_of_user, pl.pose_user_of_int, pl.jopt_of_user, pl.N);
  const std::vector<int32_t> order = number_points(in, threads, pl);
  clk.lap("validate + order + owners");
  PointObs point_obs = build_point_obs(in, threads, pl);
  clk.lap("per-point observation lists");
  group_landmarks(in, knobs, threads, point_obs, clk, pl);
  clk.lap("covisibility groups");
  if (knobs.interleave) interleave_windows(knobs, pl);
  append_fixed_points(in, order, pl);
  clk.lap("interleave + fixed points");
  err = build_landmark_major(threads, point_obs, pl);
  if (!err.empty()) return err;
  // (the per-point lists are not needed any more: their 140 MB go back to the system on a
  //  side thread while the remaining phases run)
  struct Reaper {
    std::thread t;
    ~Reaper() {
      if (t.joinable()) t.join();
    }
  } reaper;
  reaper.t = std::thread([po = std::move(point_obs)]() mutable { po = PointObs(); });
  clk.lap("landmark-major list");
  build_pose_major(pl);
  clk.lap("pose-major list");
  err = build_schur_structure(in, knobs, pl);
  if (!err.empty()) return err;
  clk.lap("Schur structure");
  build_backsub_chunks(pl);
  finish_lin_grp_bookkeeping(pl);
  clk.lap("chunks + bookkeeping");
  return std::string();
}


// Tile pattern of S for tiles of `poses_per_tile` consecutive optimised poses
// (global: every shard factors the same matrix).
void tile_pattern(const Plan &pl, int poses_per_tile, int &ncb,
                  std::vector<uint8_t> &adj) {
  ncb = std::max(1, (pl.N + poses_per_tile - 1) / poses_per_tile);
  adj.assign((size_t)ncb * ncb, 0);
  for (int t = 0; t < ncb; ++t) adj[(size_t)t * ncb + t] = 1;
  for (int64_t bk = 0; bk < pl.B; ++bk) {
    const int a = pl.sblk_j[bk] / poses_per_tile, b = pl.sblk_k[bk] / poses_per_tile;
    adj[(size_t)a * ncb + b] = 1;
    adj[(size_t)b * ncb + a] = 1;
  }
}

}  // namespace ba
