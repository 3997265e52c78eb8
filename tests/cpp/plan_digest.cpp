// Digest of the whole work plan (csrc/ba_plan.cpp) over a fixed list of named cases,
// compiled with g++ by tests/test_plan_invariants.py and compared line by line with
// tests/cpp/plan_digest_expected.txt, which holds this program's output against an EARLIER
// commit's planner (named in that file's first line): the planner may be rearranged, what
// it decides may not change unseen.  Uses the public interface of ba_plan.h only; the knobs
// of every case are set here, not through the environment.
//
//   plan_digest                  one line per case, exit 1 when a counter that the list
//                                must reach stays zero
//   plan_digest --time [threads] wall time of build_plan alone on two scenes of the
//                                benchmark's shape (1000 poses, 500 000 landmarks, windows
//                                of 5 in 2 cameras; the second with 15 % dropout)
//
// Scene (as tests/cpp/plan_check.cpp): every landmark is seen by `win` consecutive poses in
// `n_cam` cameras, `drop` per cent of the observations dropped pseudo-randomly, a few
// landmarks seen by every pose and a few never observed; the first three poses and every
// 97th point fixed.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ba_plan.h"
#include "plan_digest.h"

namespace {

struct Scene {
  int n_pose, n_pt, win, n_cam, drop;
  int n_cam_declared = 0;  // > 0: PlanInput::n_cam (the observations still use cameras [0, n_cam))
  int fixed_tail_pct = 0;  // the last so many per cent of the points are fixed: a shard that owns no optimisable landmark
  bool specials = true;    // every-pose and never-observed landmarks
  std::vector<uint8_t> pf, qf;
  std::vector<int32_t> oc, op, oq;
  std::vector<double> uv;
  Scene(int n_pose_, int n_pt_, int win_, int n_cam_, int drop_ = 0) : n_pose(n_pose_), n_pt(n_pt_), win(win_), n_cam(n_cam_), drop(drop_) {}
  ba::PlanInput input() {
    pf.assign(n_pose, 0);
    qf.assign(n_pt, 0);
    for (int k = 0; k < 3; ++k) pf[k] = 1;
    for (int q = 0; q < n_pt; q += 97) qf[q] = 1;
    for (int q = (int)((int64_t)n_pt * (100 - fixed_tail_pct) / 100); q < n_pt; ++q) qf[q] = 1;
    oc.clear(), op.clear(), oq.clear(), uv.clear();
    for (int q = 0; q < n_pt; ++q) {
      if (specials && q % 1013 == 5) continue;  // never observed
      int j0 = (int)((long long)q * (n_pose - win + 1) / n_pt), w = win;
      if (specials && q % 4001 == 7) {  // seen by every pose
        j0 = 0;
        w = n_pose;
      }
      for (int j = j0; j < j0 + w; ++j)
        for (int c = 0; c < n_cam; ++c) {
          const unsigned hsh = (unsigned)(q * 2654435761u) ^ (unsigned)(j * 40503u + c * 977u);
          if (drop > 0 && !(j == j0 && c == 0) && (int)((hsh >> 7) % 100u) < drop) continue;
          oc.push_back(c), op.push_back(j), oq.push_back(q), uv.push_back(q), uv.push_back(j + 0.25 * c);
        }
    }
    ba::PlanInput in;
    in.n_cam = n_cam_declared > 0 ? n_cam_declared : n_cam;
    in.n_pose = n_pose, in.pose_fixed = pf.data(), in.n_pt = n_pt, in.pt_fixed = qf.data();
    in.n_obs = (int64_t)oc.size(), in.obs_cam = oc.data(), in.obs_pose = op.data(), in.obs_pt = oq.data(), in.obs_uv = uv.data();
    return in;
  }
};

ba::PlanKnobs knobs_with(void (*set)(ba::PlanKnobs &) = nullptr) {
  ba::PlanKnobs k;
  k.threads = 4;
  if (set) set(k);
  return k;
}

// What the list of cases must reach at least once (summed over the cases).
struct Reached {
  long masked = 0, joined = 0, g32 = 0, g64 = 0, g128 = 0, runs = 0, split_runs = 0, tri = 0, rel_only = 0, empty_shard = 0;
} g_reached;

// members of masked groups whose own pose span (user indices of the poses that really
// observe them) is narrower than their group's union: leftovers of the span buckets that
// joined a group whose union contains their pattern
long joined_leftovers(const ba::Plan &pl) {
  long n = 0;
  for (const ba::Plan::GrpRange &g : pl.grp_range) {
    if (!g.masked) continue;
    int lo = INT32_MAX, hi = -1;
    for (int e = 0; e < g.no; ++e) {
      const int u = pl.pose_user_of_int[(size_t)(pl.grp_upat[g.upat0 + e] >> 32)];
      lo = std::min(lo, u), hi = std::max(hi, u);
    }
    for (int l = g.l0; l < g.l0 + g.nl; ++l) {
      int a = INT32_MAX, b = -1;
      for (int64_t s = pl.lm_obs_ptr[l]; s < pl.lm_obs_ptr[l + 1]; ++s) {
        if (std::isnan(pl.obs_uv[2 * s])) continue;
        const int u = pl.pose_user_of_int[pl.obs_idx[4 * s + 1]];
        a = std::min(a, u), b = std::max(b, u);
      }
      n += a != lo || b != hi;
    }
  }
  return n;
}

// super-runs that hold one pose-group class of their landmarks, not all their triples
long split_class_runs(const ba::Plan &pl) {
  long n = 0;
  for (const ba::Plan::SupDesc &sd : pl.sup_desc) {
    bool part = false;
    for (int c = sd.chunk_begin; c < sd.chunk_end; ++c) {
      const ba::Plan::ChunkDesc &cd = pl.chunk_desc[c];
      int64_t all = 0;
      for (int l = cd.l0; l < cd.l0 + cd.nl; ++l) {
        const int64_t d = pl.lm_pair_ptr[l + 1] - pl.lm_pair_ptr[l];
        all += d * (d + 1) / 2;
      }
      part = part || cd.nt != all;
    }
    n += part;
  }
  return n;
}

uint64_t run_case(const char *name, const ba::PlanInput &in, const ba::PlanKnobs &knobs) {
  ba::Plan pl;
  const std::string err = ba::build_plan(in, knobs, pl);
  if (!err.empty()) {
    std::printf("case %s: error \"%s\"\n", name, err.c_str());
    return 0;
  }
  long exact = 0, masked = 0;
  for (const ba::Plan::GrpRange &g : pl.grp_range) (g.masked ? masked : exact)++;
  const long joined = joined_leftovers(pl), split_runs = split_class_runs(pl);
  const uint64_t h = plan_digest::of(pl);
  std::printf("case %s: digest %016llx tiles1 %016llx tiles4 %016llx N %d M %d grouped %d exact %ld masked %ld joined %ld "
              "grp32 %zu grp64 %zu grp128 %zu lin %zu runs %zu split_runs %ld chunks %zu tri %zu rel_only %lld pair_pad %lld\n",
              name, (unsigned long long)h, (unsigned long long)plan_digest::of_tiles(pl, 1),
              (unsigned long long)plan_digest::of_tiles(pl, 4), pl.N, pl.M, pl.M_grp, exact, masked, joined, pl.grp32.size(),
              pl.grp64.size(), pl.grp128.size(), pl.lin_desc.size(), pl.sup_desc.size(), split_runs, pl.chunk_desc.size(),
              pl.tri_p.size(), (long long)pl.n_rel_only, (long long)pl.n_pair_pad);
  g_reached.masked += masked, g_reached.joined += joined, g_reached.g32 += (long)pl.grp32.size();
  g_reached.g64 += (long)pl.grp64.size(), g_reached.g128 += (long)pl.grp128.size(), g_reached.runs += (long)pl.sup_desc.size();
  g_reached.split_runs += split_runs, g_reached.tri += (long)pl.tri_p.size(), g_reached.rel_only += (long)pl.n_rel_only;
  g_reached.empty_shard += pl.M == 0;
  return h;
}

uint64_t run_case(const char *name, Scene sc, const ba::PlanKnobs &knobs = knobs_with()) { return run_case(name, sc.input(), knobs); }

// an error path: the returned string, and whether the caller's plan was left as it was
void run_error(const char *name, const ba::PlanInput &in, int threads) {
  ba::Plan pl;
  pl.n_cam = -7;
  pl.owner.assign(3, 5);
  ba::PlanKnobs knobs;
  knobs.threads = threads;
  const std::string err = ba::build_plan(in, knobs, pl);
  std::printf("error %s: \"%s\" plan %s\n", name, err.c_str(), pl.n_cam == -7 && pl.owner.size() == 3 ? "untouched" : "reset");
}

void shard_cases() {
  // world 2 and 3 at every rank.  With the last 40 % of the points fixed, the last of three
  // shards owns the never-observed landmarks only (they are last in the locality order), and
  // in the scene without those no optimisable landmark at all
  struct Variant {
    const char *name;
    int fixed_tail_pct;
    bool specials;
  };
  const Variant variants[] = {{"all_free", 0, true}, {"fixed_tail", 40, true}, {"fixed_tail.plain", 40, false}};
  for (int world = 2; world <= 3; ++world)
    for (int rank = 0; rank < world; ++rank)
      for (const Variant &v : variants) {
        Scene sc(60, 3000, 5, 2, 15);
        sc.fixed_tail_pct = v.fixed_tail_pct;
        sc.specials = v.specials;
        ba::PlanInput in = sc.input();
        in.rank = rank, in.world = world;
        char name[64];
        std::snprintf(name, sizeof name, "world%d.rank%d.%s", world, rank, v.name);
        run_case(name, in, knobs_with());
      }
}

void relative_cases() {
  // 60 poses, the first three fixed, windows of 5 and no landmark that every pose sees: user
  // pose u >= 3 is optimised pose u - 3; only poses less than 5 apart share landmarks
  struct Rel {
    const char *name;
    std::vector<int32_t> j, k;
  };
  const Rel sets[] = {
      {"rel.covisible_block", {10}, {12}},
      {"rel.factor_only_block", {10}, {50}},
      {"rel.opt_fixed", {1, 20}, {30, 0}},
      {"rel.same_factor_twice", {10, 10}, {50, 50}},
      {"rel.j_above_k", {50, 12}, {10, 11}},
      {"rel.all", {10, 10, 1, 20, 10, 50, 12, 50, 33, 4}, {12, 50, 30, 0, 50, 10, 11, 10, 59, 58}},
  };
  for (const Rel &r : sets) {
    Scene sc(60, 3000, 5, 2);
    sc.specials = false;
    ba::PlanInput in = sc.input();
    in.n_rel = (int64_t)r.j.size(), in.rel_j = r.j.data(), in.rel_k = r.k.data();
    run_case(r.name, in, knobs_with());
    if (std::strcmp(r.name, "rel.all") != 0) continue;
    for (int rank = 0; rank < 2; ++rank) {
      in.rank = rank, in.world = 2;
      run_case(rank == 0 ? "rel.all.world2.rank0" : "rel.all.world2.rank1", in, knobs_with());
    }
    Scene sd(60, 3000, 5, 2, 15);  // (masked groups beside the factors)
    sd.specials = false;
    ba::PlanInput ind = sd.input();
    ind.n_rel = (int64_t)r.j.size(), ind.rel_j = r.j.data(), ind.rel_k = r.k.data();
    run_case("rel.all.dropout", ind, knobs_with());
  }
}

int thread_cases() {
  int bad = 0;
  const Scene scenes[] = {Scene(120, 30000, 5, 2, 15), Scene(90, 2000, 37, 2), Scene(60, 20000, 20, 1, 15)};
  const char *names[][2] = {{"threads1.stereo_dropout", "threads7.stereo_dropout"},
                            {"threads1.four_pose_groups", "threads7.four_pose_groups"},
                            {"threads1.wide_dropout", "threads7.wide_dropout"}};
  for (int s = 0; s < 3; ++s) {
    const uint64_t h1 = run_case(names[s][0], scenes[s], knobs_with([](ba::PlanKnobs &k) { k.threads = 1; }));
    const uint64_t h7 = run_case(names[s][1], scenes[s], knobs_with([](ba::PlanKnobs &k) { k.threads = 7; }));
    if (h1 != h7) {
      std::printf("FAIL: %s and %s differ\n", names[s][0], names[s][1]);
      ++bad;
    }
  }
  return bad;
}

void error_cases() {
  Scene sc(40, 6000, 5, 2);  // 59 k observations: three thread ranges of >= 4096
  const ba::PlanInput ok = sc.input();
  ba::PlanInput in = ok;
  in.n_cam = 0;
  run_error("no_cameras", in, 1);
  in = ok, in.n_pose = 0;
  run_error("no_poses", in, 1);
  in = ok, in.n_pt = 0;
  run_error("no_points", in, 1);
  in = ok, in.n_cam = 0, in.n_pose = 0, in.n_pt = 0;
  run_error("nothing_at_all", in, 1);
  in = ok, in.rank = 2, in.world = 2;
  run_error("rank_equals_world", in, 1);
  in = ok, in.rank = -1;
  run_error("negative_rank", in, 1);
  in = ok, in.world = 0;
  run_error("world_zero", in, 1);
  // an invalid camera, pose and point index on three observations: the smallest index is reported
  const int64_t n = ok.n_obs, at[3] = {n / 6, n / 2, 5 * n / 6};  // one in each of three threads' ranges
  const char *kinds = "cpq";  // camera, pose, point
  const int orders[3][3] = {{0, 1, 2}, {2, 0, 1}, {1, 2, 0}};
  for (const auto &ord : orders)
    for (int threads : {1, 3}) {
      std::vector<int32_t> oc = sc.oc, op = sc.op, oq = sc.oq;
      char name[64];
      std::snprintf(name, sizeof name, "invalid_index.order_%c%c%c.threads%d", kinds[ord[0]], kinds[ord[1]], kinds[ord[2]], threads);
      for (int t = 0; t < 3; ++t) {
        if (ord[t] == 0) oc[at[t]] = t == 1 ? -1 : sc.n_cam;
        if (ord[t] == 1) op[at[t]] = t == 1 ? -1 : sc.n_pose;
        if (ord[t] == 2) oq[at[t]] = t == 1 ? -1 : sc.n_pt;
      }
      in = ok, in.obs_cam = oc.data(), in.obs_pose = op.data(), in.obs_pt = oq.data();
      run_error(name, in, threads);
    }
  // all three on ONE observation: camera, then pose, then point
  {
    std::vector<int32_t> oc = sc.oc, op = sc.op, oq = sc.oq;
    oc[at[1]] = -1, op[at[1]] = sc.n_pose, oq[at[1]] = sc.n_pt;
    in = ok, in.obs_cam = oc.data(), in.obs_pose = op.data(), in.obs_pt = oq.data();
    run_error("invalid_index.one_observation", in, 3);
    oc[at[1]] = 0;
    run_error("invalid_index.one_observation.pose_and_point", in, 3);
  }
}

int time_mode(int threads) {
  for (int drop : {0, 15}) {
    Scene sc(1000, 500000, 5, 2, drop);
    sc.specials = false;
    const ba::PlanInput in = sc.input();
    ba::PlanKnobs knobs;
    knobs.threads = threads;
    ba::Plan pl;
    const auto t0 = std::chrono::steady_clock::now();
    const std::string err = ba::build_plan(in, knobs, pl);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!err.empty()) {
      std::printf("build_plan: %s\n", err.c_str());
      return 1;
    }
    std::printf("time dropout%d: build_plan %.1f ms (observations %lld, pairs %lld, digest %016llx)\n", drop, ms,
                (long long)pl.n_obs, (long long)pl.P, (unsigned long long)plan_digest::of(pl));
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "--time") == 0) return time_mode(argc > 2 ? atoi(argv[2]) : 0);
  using K = ba::PlanKnobs;
  // ---- the shapes of tests/test_plan_invariants.py test_plan_invariants ----
  const auto no_groups = [](K &k) { k.groups = false; };
  run_case("stereo_windows", Scene(120, 30000, 5, 2));
  run_case("mono_wide_windows", Scene(40, 3000, 9, 1));
  run_case("large_groups", Scene(30, 40000, 4, 1));
  run_case("stereo_windows.no_groups", Scene(120, 30000, 5, 2), knobs_with(no_groups));
  run_case("mono_wide_windows.no_groups", Scene(40, 3000, 9, 1), knobs_with(no_groups));
  run_case("plain_order", Scene(60, 8000, 5, 2), knobs_with([](K &k) { k.interleave = false, k.groups = false; }));
  run_case("tiny_runs", Scene(30, 400, 5, 2), knobs_with([](K &k) { k.sup_cap = 7, k.groups = false; }));
  run_case("slot_limited_runs", Scene(200, 6000, 3, 3), knobs_with([](K &k) { k.sup_cap = 1000, k.groups = false; }));
  run_case("groups_beside_runs", Scene(200, 6000, 3, 3));
  run_case("windows20", Scene(60, 3000, 20, 1));
  run_case("windows20.no_split", Scene(60, 3000, 20, 1), knobs_with([](K &k) { k.split = false; }));
  run_case("windows20.no_groups", Scene(60, 3000, 20, 1), knobs_with(no_groups));
  run_case("windows20.no_groups.no_split", Scene(60, 3000, 20, 1), knobs_with([](K &k) { k.groups = false, k.split = false; }));
  run_case("stereo16", Scene(60, 3000, 16, 2));
  run_case("windows20.dropout", Scene(60, 3000, 20, 1, 15));
  run_case("four_pose_groups", Scene(90, 2000, 37, 2), knobs_with(no_groups));
  run_case("lin_steps2", Scene(120, 30000, 5, 2), knobs_with([](K &k) { k.lin_steps = 2; }));
  run_case("no_lin_groups", Scene(120, 30000, 5, 2), knobs_with([](K &k) { k.lin_groups = false; }));
  run_case("stereo_dropout", Scene(120, 30000, 5, 2, 15));
  run_case("mono_wide_dropout", Scene(40, 3000, 9, 1, 25));
  run_case("stereo_dropout.no_superset", Scene(120, 30000, 5, 2, 15), knobs_with([](K &k) { k.superset = false; }));
  // ---- every knob off / set once more, on a scene that has exact groups, super-runs and
  // split landmarks side by side (dropout without superset groups) ----
  const Scene mixed(60, 6000, 5, 2, 15);
  run_case("mixed", mixed, knobs_with([](K &k) { k.superset = false; }));
  run_case("mixed.no_split", mixed, knobs_with([](K &k) { k.superset = false, k.split = false; }));
  run_case("mixed.sup_cap40", mixed, knobs_with([](K &k) { k.superset = false, k.sup_cap = 40; }));
  // (the interleave permutes windows of one run's landmarks: the identity at the smallest run size)
  run_case("mixed.sup_cap40.no_interleave", mixed, knobs_with([](K &k) { k.superset = false, k.sup_cap = 40, k.interleave = false; }));
  run_case("mixed.lin_steps1", mixed, knobs_with([](K &k) { k.superset = false, k.lin_steps = 1; }));
  run_case("mixed.no_lin_groups", mixed, knobs_with([](K &k) { k.lin_groups = false; }));
  run_case("mixed.superset", mixed);
  {
    Scene sc(60, 3000, 5, 2, 15);  // 65536 cameras: no slim record, no k_lin_grp pieces
    sc.n_cam_declared = 65536;
    run_case("dropout.cameras65536", sc);
  }
  shard_cases();
  relative_cases();
  int bad = thread_cases();
  error_cases();
  const struct {
    const char *what;
    long n;
  } must[] = {{"masked groups", g_reached.masked},   {"leftovers that joined a group", g_reached.joined},
              {"grp32 pieces", g_reached.g32},       {"grp64 pieces", g_reached.g64},
              {"grp128 pieces", g_reached.g128},     {"super-runs", g_reached.runs},
              {"split-class runs", g_reached.split_runs}, {"global triple list", g_reached.tri},
              {"factor-only blocks", g_reached.rel_only}, {"shards without an optimisable landmark", g_reached.empty_shard}};
  for (const auto &m : must) {
    std::printf("reached %s: %ld\n", m.what, m.n);
    if (m.n == 0) {
      std::printf("FAIL: no case reaches %s\n", m.what);
      ++bad;
    }
  }
  std::printf("%s\n", bad ? "PLAN DIGEST FAILED" : "PLAN DIGEST OK");
  return bad ? 1 : 0;
}
