// Host-only check of the planner's part of the relative-pose factors of the handle path
// (csrc/ba_plan.cpp, PlanInput::rel_j / rel_k), compiled with g++ by
// tests/test_relative_plan.py.  Scene: every landmark is seen by `win` consecutive poses in
// two cameras, the first three poses fixed.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "ba_plan.h"

static int g_fail = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (g_fail < 20) {                         \
        std::printf("FAIL line %d: ", __LINE__); \
        std::printf(__VA_ARGS__);                \
        std::printf("\n");                       \
      }                                          \
      ++g_fail;                                  \
    }                                            \
  } while (0)

template <class V>
static bool same(const V &a, const V &b) {
  return a.size() == b.size() && std::equal(a.begin(), a.end(), b.begin());
}

// every array a plan had before the factors came
static bool same_plan(const ba::Plan &a, const ba::Plan &b) {
  return a.N == b.N && a.M == b.M && a.P == b.P && a.T == b.T && a.B == b.B && same(a.sblk_j, b.sblk_j) &&
         same(a.sblk_k, b.sblk_k) && same(a.diag_blk, b.diag_blk) && same(a.pose_int_of_user, b.pose_int_of_user) &&
         same(a.pt_int_of_user, b.pt_int_of_user) && same(a.obs_idx, b.obs_idx) && same(a.lm_pair_ptr, b.lm_pair_ptr) &&
         same(a.pair_pose, b.pair_pose) && same(a.sblk_tri_ptr, b.sblk_tri_ptr) && same(a.tri_p, b.tri_p) &&
         same(a.tri_q, b.tri_q) && same(a.tchunk_blk, b.tchunk_blk) && same(a.slot_blk, b.slot_blk) &&
         same(a.ltri, b.ltri) && same(a.chunk_sp, b.chunk_sp) && same(a.sup_lane, b.sup_lane) &&
         same(a.blk_contrib_ptr, b.blk_contrib_ptr) && same(a.contrib_slot, b.contrib_slot) &&
         same(a.bchunk_lm, b.bchunk_lm) && same(a.grp_pat, b.grp_pat) && same(a.pose_gpart, b.pose_gpart) &&
         a.sup_desc.size() == b.sup_desc.size() && a.chunk_desc.size() == b.chunk_desc.size() &&
         a.grp32.size() == b.grp32.size() && a.grp64.size() == b.grp64.size() && a.grp128.size() == b.grp128.size() &&
         a.lin_desc.size() == b.lin_desc.size();
}

int main(int argc, char **argv) {
  const int n_pose = argc > 1 ? atoi(argv[1]) : 60, n_pt = argc > 2 ? atoi(argv[2]) : 3000;
  const int win = argc > 3 ? atoi(argv[3]) : 5, n_cam = 2, n_fixed = 3;
  std::vector<uint8_t> pf(n_pose, 0), qf(n_pt, 0);
  for (int k = 0; k < n_fixed; ++k) pf[k] = 1;
  std::vector<int32_t> oc, op, oq;
  std::vector<double> uv;
  for (int q = 0; q < n_pt; ++q) {
    const int j0 = (int)((long long)q * (n_pose - win + 1) / n_pt);
    for (int j = j0; j < j0 + win; ++j)
      for (int c = 0; c < n_cam; ++c) {
        oc.push_back(c); op.push_back(j); oq.push_back(q); uv.push_back(q); uv.push_back(j);
      }
  }
  ba::PlanInput in;
  in.n_cam = n_cam; in.n_pose = n_pose; in.pose_fixed = pf.data(); in.n_pt = n_pt; in.pt_fixed = qf.data();
  in.n_obs = (int64_t)oc.size(); in.obs_cam = oc.data(); in.obs_pose = op.data(); in.obs_pt = oq.data(); in.obs_uv = uv.data();
  const ba::PlanKnobs knobs = ba::Knobs::from_env().plan;
  ba::Plan p0;
  std::string err = ba::build_plan(in, knobs, p0);
  CHECK(err.empty(), "build_plan: %s", err.c_str());
  if (!err.empty()) return 1;
  CHECK(p0.n_rel == 0 && p0.n_rel_only == 0 && p0.rel_jk.empty() && p0.rel_pptr.empty() && p0.rel_plist.empty() &&
            p0.rel_blk.empty() && p0.rel_bptr.empty() && p0.rel_blist.empty(),
        "a plan without factors has no factor lists");

  // ---- factors to a fixed pose only: no block is added, every other array stays as it is
  {
    std::vector<int32_t> rj = {0, n_fixed + 4, n_pose - 1}, rk = {n_fixed + 1, 1, 2};
    ba::PlanInput inf = in;
    inf.n_rel = (int64_t)rj.size(); inf.rel_j = rj.data(); inf.rel_k = rk.data();
    ba::Plan pf1;
    err = ba::build_plan(inf, knobs, pf1);
    CHECK(err.empty(), "build_plan: %s", err.c_str());
    CHECK(same_plan(p0, pf1), "factors to fixed poses change the plan");
    CHECK(pf1.rel_blk.empty() && pf1.rel_bptr.size() == 1 && pf1.n_rel_only == 0, "a fixed pose couples no block");
    CHECK((int)pf1.rel_plist.size() == 3, "one list entry per optimisable end");
  }

  // ---- the full set: chain, far pairs in both orientations, duplicates, fixed ends
  std::vector<int32_t> rj, rk;
  for (int q = n_fixed - 1; q < n_pose - 1; ++q) { rj.push_back(q + 1); rk.push_back(q); }   // the first has k fixed
  const int far[4][2] = {{n_pose - 2, n_fixed + 1}, {n_fixed + 2, n_pose - 1}, {n_pose - 4, n_pose / 3}, {n_pose / 4, n_pose - 6}};
  for (auto &f : far) { rj.push_back(f[0]); rk.push_back(f[1]); }
  rj.push_back(0); rk.push_back(n_fixed + 3);                                                // j fixed
  rj.push_back(n_fixed + 5); rk.push_back(n_fixed + 7);                                      // one pair twice,
  rj.push_back(n_fixed + 7); rk.push_back(n_fixed + 5);                                      // both orientations
  rj.push_back(n_pose - 2); rk.push_back(n_fixed + 1);                                       // a far pair again
  const int F = (int)rj.size();
  ba::PlanInput inr = in;
  inr.n_rel = F; inr.rel_j = rj.data(); inr.rel_k = rk.data();
  ba::Plan pl;
  err = ba::build_plan(inr, knobs, pl);
  CHECK(err.empty(), "build_plan: %s", err.c_str());
  const int N = pl.N;
  CHECK(N == p0.N && pl.n_rel == F && (int)pl.rel_jk.size() == 4 * F, "sizes");
  // blocks: sorted, unique, every diagonal leads its row
  std::map<std::pair<int, int>, int> blk_of;
  for (int64_t b = 0; b < pl.B; ++b) {
    CHECK(pl.sblk_j[b] <= pl.sblk_k[b] && pl.sblk_k[b] < N, "upper block");
    CHECK(blk_of.emplace(std::make_pair(pl.sblk_j[b], pl.sblk_k[b]), (int)b).second, "block (%d, %d) twice", pl.sblk_j[b], pl.sblk_k[b]);
  }
  for (int j = 0; j < N; ++j) CHECK(pl.sblk_j[pl.diag_blk[j]] == j && pl.sblk_k[pl.diag_blk[j]] == j, "diag_blk");
  std::map<std::pair<int, int>, int> blk0;
  for (int64_t b = 0; b < p0.B; ++b) blk0[{p0.sblk_j[b], p0.sblk_k[b]}] = (int)b;
  // per factor: its record, its block (exactly once), its place in the lists
  std::map<int, std::vector<int>> want_blist;
  std::vector<std::vector<int>> want_plist(N);
  int64_t only = 0;
  std::vector<int> only_seen;
  for (int f = 0; f < F; ++f) {
    const int a = pl.pose_int_of_user[rj[f]], b = pl.pose_int_of_user[rk[f]];
    CHECK(pl.rel_jk[4 * f] == a && pl.rel_jk[4 * f + 1] == b, "factor %d poses", f);
    CHECK(pl.rel_jk[4 * f + 2] == (a < N ? a : -1) && pl.rel_jk[4 * f + 3] == (b < N ? b : -1), "factor %d opt index", f);
    CHECK((a < N) == !pf[rj[f]] && (b < N) == !pf[rk[f]], "optimisable poses come first");
    if (a < N) want_plist[a].push_back(f << 1);
    if (b < N) want_plist[b].push_back((f << 1) | 1);
    if (a >= N || b >= N) continue;
    const auto it = blk_of.find({std::min(a, b), std::max(a, b)});
    CHECK(it != blk_of.end(), "factor %d has no block", f);
    if (it == blk_of.end()) continue;
    want_blist[it->second].push_back((f << 1) | (a > b ? 1 : 0));
    if (!blk0.count(it->first) && std::find(only_seen.begin(), only_seen.end(), it->second) == only_seen.end()) {
      only_seen.push_back(it->second);
      ++only;
      CHECK(pl.blk_contrib_ptr[it->second] == pl.blk_contrib_ptr[it->second + 1], "a factor-only block has contributions");
      CHECK(pl.sblk_tri_ptr[it->second] == pl.sblk_tri_ptr[it->second + 1], "a factor-only block has triples");
    }
  }
  CHECK(only == pl.n_rel_only && only >= 3, "blocks that exist only because of a factor: %lld / %lld", (long long)only, (long long)pl.n_rel_only);
  CHECK(pl.B == p0.B + only, "every new pair is a block exactly once");
  for (auto &kv : blk0) CHECK(blk_of.count(kv.first), "a covisibility block is gone");
  // coupled blocks: ascending ids, lists in input order, orientation flags
  CHECK(pl.rel_blk.size() == want_blist.size() && pl.rel_bptr.size() == pl.rel_blk.size() + 1, "coupled blocks");
  size_t t = 0;
  for (auto &kv : want_blist) {
    if (t >= pl.rel_blk.size()) break;
    CHECK(pl.rel_blk[t] == kv.first, "coupled block %zu", t);
    const std::vector<int> got(pl.rel_blist.begin() + pl.rel_bptr[t], pl.rel_blist.begin() + pl.rel_bptr[t + 1]);
    CHECK(got == kv.second, "list of coupled block %zu", t);
    ++t;
  }
  bool both = false, twice = false;
  for (auto &kv : want_blist) {
    if (kv.second.size() < 2) continue;
    const bool flip = (kv.second[0] ^ kv.second[1]) & 1;
    both |= flip;     // the pair named in both orientations
    twice |= !flip;   // the far pair named twice
  }
  CHECK(both && twice, "duplicates and both orientations share one block");
  CHECK((int)pl.rel_pptr.size() == N + 1, "pose pointers");
  for (int j = 0; j < N && (int)pl.rel_pptr.size() == N + 1; ++j) {
    const std::vector<int> got(pl.rel_plist.begin() + pl.rel_pptr[j], pl.rel_plist.begin() + pl.rel_pptr[j + 1]);
    CHECK(got == want_plist[j], "list of pose %d", j);
  }
  // the tile pattern couples the tiles of every coupled pair, for both tile orders
  for (int ppt : {5, 10}) {
    int ncb = 0, ncb0 = 0;
    std::vector<uint8_t> adj, adj0;
    ba::tile_pattern(pl, ppt, ncb, adj);
    ba::tile_pattern(p0, ppt, ncb0, adj0);
    CHECK(ncb == ncb0, "tiles");
    bool grew = false;
    for (int b : pl.rel_blk) {
      const int ta = pl.sblk_j[b] / ppt, tb = pl.sblk_k[b] / ppt;
      CHECK(adj[(size_t)ta * ncb + tb] && adj[(size_t)tb * ncb + ta], "tiles %d, %d are not coupled", ta, tb);
      grew |= !adj0[(size_t)ta * ncb + tb];
    }
    CHECK(grew, "a far pair couples tiles that no landmark couples");
  }
  // the rest of the plan is the plan without factors, but for the block numbering
  CHECK(same(pl.obs_idx, p0.obs_idx) && same(pl.pair_pose, p0.pair_pose) && same(pl.ltri, p0.ltri) &&
            pl.contrib_slot.size() == p0.contrib_slot.size() && pl.T == p0.T && pl.P == p0.P,
        "the factors change more than the block list");
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("N %d B %lld (+%lld) coupled %zu factors %d OK\n", N, (long long)pl.B, (long long)only, pl.rel_blk.size(), F);
  return 0;
}
