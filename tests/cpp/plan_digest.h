// plan_digest.h — one 64-bit hash over EVERY member of ba::Plan (csrc/ba_plan.h).
//
// A NEW MEMBER OF ba::Plan MUST BE ADDED HERE: tests/cpp/plan_digest.cpp compares the
// digest of a list of cases with the values recorded from an earlier commit
// (tests/cpp/plan_digest_expected.txt), and tests/cpp/plan_check.cpp prints it for the
// 1-thread / 7-thread comparison.  A member that is not folded in is a member that a
// planner change can alter unseen.
//
// Vectors are hashed with their length, records field by field (never as raw bytes:
// Plan::GrpRange has four bytes of implicit padding that the planner leaves
// uninitialised), doubles by bit pattern.
#ifndef PLAN_DIGEST_H_
#define PLAN_DIGEST_H_

#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "ba_plan.h"

namespace plan_digest {

struct Hasher {
  uint64_t h = 1469598103934665603ull;
  void word(uint64_t v) { h = (h ^ v) * 0x100000001b3ull + (h >> 29); }
  template <class T>
  void num(T v) {  // integral members sign-extended, doubles by bit pattern
    if constexpr (std::is_floating_point<T>::value) {
      static_assert(sizeof(T) == 8, "double");
      uint64_t b;
      std::memcpy(&b, &v, 8);
      word(b);
    } else {
      word((uint64_t)(int64_t)v);
    }
  }
  template <class T, class A>
  void vec(const std::vector<T, A> &v) {
    word((uint64_t)v.size());
    for (const T &x : v) num(x);
  }
};

inline uint64_t of(const ba::Plan &pl) {
  Hasher s;
  // ---- sizes ----
  s.num(pl.n_cam), s.num(pl.n_pose), s.num(pl.N), s.num(pl.n_pt_global), s.num(pl.M_global), s.num(pl.n_pt), s.num(pl.M);
  s.num(pl.n_obs_global), s.num(pl.n_obs), s.num(pl.n_obs_opt), s.num(pl.P), s.num(pl.n_pobs), s.num(pl.T), s.num(pl.B);
  // ---- index maps ----
  s.vec(pl.pose_int_of_user), s.vec(pl.pose_user_of_int), s.vec(pl.jopt_of_user);
  s.vec(pl.pt_int_of_user), s.vec(pl.pt_user_of_int), s.vec(pl.iopt_of_user), s.vec(pl.owner);
  // ---- landmark-major observations, pairs ----
  s.vec(pl.obs_idx), s.vec(pl.obs_cp), s.vec(pl.obs_uv), s.vec(pl.lm_obs_ptr);
  s.vec(pl.lm_pair_ptr), s.vec(pl.pair_pose), s.vec(pl.pair_lm);
  // ---- pose-major observations ----
  s.vec(pl.pobs_idx), s.vec(pl.pobs_uv), s.vec(pl.pose_obs_ptr);
  s.vec(pl.achunk_pose), s.vec(pl.achunk_begin), s.vec(pl.achunk_end), s.vec(pl.pose_achunk_ptr);
  // ---- Schur blocks, global triple list ----
  s.vec(pl.sblk_j), s.vec(pl.sblk_k), s.vec(pl.diag_blk), s.vec(pl.sblk_tri_ptr), s.vec(pl.tri_p), s.vec(pl.tri_q);
  s.vec(pl.tchunk_blk), s.vec(pl.tchunk_begin), s.vec(pl.tchunk_end), s.vec(pl.sblk_tchunk_ptr);
  // ---- super-runs ----
  s.word((uint64_t)pl.sup_desc.size());
  for (const ba::Plan::SupDesc &d : pl.sup_desc) s.num(d.s0), s.num(d.ns), s.num(d.chunk_begin), s.num(d.chunk_end);
  s.vec(pl.sup_lane);
  s.word((uint64_t)pl.chunk_desc.size());
  for (const ba::Plan::ChunkDesc &d : pl.chunk_desc)
    s.num(d.p0), s.num(d.tb), s.num(d.sp), s.num(d.l0), s.num(d.nl), s.num(d.np), s.num(d.nt);
  s.vec(pl.chunk_sp), s.vec(pl.slot_blk), s.vec(pl.ltri), s.vec(pl.blk_contrib_ptr), s.vec(pl.contrib_slot), s.vec(pl.bchunk_lm);
  // ---- covisibility groups ----
  s.num(pl.M_grp), s.num((int64_t)pl.lin_groups);
  s.vec(pl.grp_upat), s.vec(pl.pair_pad), s.num(pl.n_pair_pad);
  s.word((uint64_t)pl.grp_range.size());
  for (const ba::Plan::GrpRange &g : pl.grp_range) s.num(g.l0), s.num(g.nl), s.num(g.d), s.num(g.no), s.num(g.masked), s.num(g.upat0);
  s.word((uint64_t)pl.lin_desc.size());
  for (const ba::Plan::LinDesc &g : pl.lin_desc) {
    s.num(g.p0), s.num(g.o0), s.num(g.l0), s.num(g.nl), s.num(g.d), s.num(g.no);
    s.num(g.pat0), s.num(g.apart0), s.num(g.cost_idx), s.num(g.pad_);
  }
  s.num(pl.n_lin_plain);
  for (const auto *list : {&pl.grp32, &pl.grp64, &pl.grp128}) {
    s.word((uint64_t)list->size());
    for (const ba::Plan::GrpDesc &g : *list) {
      s.num(g.p0), s.num(g.l0), s.num(g.nl), s.num(g.d), s.num(g.s0);
      for (int32_t v : g.pose) s.num(v);
      for (int32_t v : g.pad_) s.num(v);
    }
  }
  s.vec(pl.grp_pat), s.num(pl.n_apart2), s.vec(pl.pose_gpart_ptr), s.vec(pl.pose_gpart), s.num(pl.n_bchunk_grp);
  // ---- relative-pose factors ----
  s.num(pl.n_rel), s.num(pl.n_rel_only);
  s.vec(pl.rel_jk), s.vec(pl.rel_pptr), s.vec(pl.rel_plist), s.vec(pl.rel_blk), s.vec(pl.rel_bptr), s.vec(pl.rel_blist);
  return s.h;
}

// the same hash over a tile pattern (ba::tile_pattern)
inline uint64_t of_tiles(const ba::Plan &pl, int poses_per_tile) {
  int ncb = 0;
  std::vector<uint8_t> adj;
  ba::tile_pattern(pl, poses_per_tile, ncb, adj);
  Hasher s;
  s.num(ncb);
  s.vec(adj);
  return s.h;
}

}  // namespace plan_digest
#endif
