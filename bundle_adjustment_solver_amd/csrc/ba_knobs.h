// ba_knobs.h — the BA_* environment variables that steer the library, as one record.
// ba_create reads it once (Knobs::from_env) and keeps it on the handle; everything below
// takes the part it needs as an argument.  A default-constructed record is the behaviour
// with a clean environment.  INTEGRATION.md has the table.  Host-only, no HIP, header only.
#ifndef BA_KNOBS_H_
#define BA_KNOBS_H_

#include <algorithm>
#include <cstdlib>

#include "ba_dense_sched.h"

namespace ba {

// What build_plan consults.
struct PlanKnobs {
  bool groups = true;      // BA_NO_GROUPS=1: no covisibility groups, every landmark through the super-runs
  bool lin_groups = true;  // BA_NO_LINGRP=1: the groups feed k_schur_grp only, not k_lin_grp
  bool superset = true;    // BA_NO_SUPERSET=1: exact groups only, no masked (union-pattern) groups
  bool interleave = true;  // BA_NO_INTERLEAVE=1: plain locality order inside a super-run window
  bool split = true;       // BA_NO_SPLIT=1: landmarks over the slot limit go to the global triple list, not to classes
  int sup_cap = 0;         // BA_SUP_CAP=n: landmarks per Schur super-run (0: schur_run_cap decides)
  int lin_steps = 0;       // BA_LIN_STEPS=n: wave steps per k_lin_grp piece (0: kLinGrpSteps)
  int threads = 0;         // BA_PLAN_THREADS=n: host threads of the planner, 1..16 (0: the hardware's, at most 16)
  bool stats = false;      // BA_PLAN_STATS set: balance of the Schur runs and the dense schedules on stderr
  bool times = false;      // BA_PLAN_TIMES set: wall time of the planner's and ba_finalize's phases on stderr
};

// What the handle consults outside the planner and the dense solve.
struct RunKnobs {
  bool force_side = false;   // BA_FORCE_SIDE=1: side stream with fork / join even where one stream would do
  bool overlap = true;       // BA_NO_OVERLAP=1: no side stream at all (seeds ba_handle::overlap)
  bool graph = false;        // BA_GRAPH=1: replay the LM iteration as a captured hipGraph (seeds ba_handle::use_graph)
  bool cost_wide = false;    // BA_COST_WIDE=1: k_cost on the 16-byte observation records (test knob)
  int cov_batch = 0;         // BA_COV_BATCH=n: columns per ba_covariance batch (0: what fits 256 MiB of workspace)
  bool stream_sync = false;  // BA_STREAM_SYNC=1: ba_stream synchronises the device after every transfer and chunk
};

// How the blocks are laid out in device memory.
struct LayoutKnobs {
  bool pair_slim = true;  // BA_PAIR_SLIM=0: the pairs of k_lin_grp's groups keep the 96-byte record {K, X_ij}, not {G, w}
  bool pair_obs = true;   // BA_PAIR_OBS=0: no "from the observation" form (ba_device.h PairObs): the slim record stays
};

struct Knobs {
  PlanKnobs plan;
  DenseKnobs dense;
  ConeKnobs cone;
  RunKnobs run;
  LayoutKnobs layout;
  static Knobs from_env();
};

inline Knobs Knobs::from_env() {
  auto is_one = [](const char *name) { const char *v = getenv(name); return v && v[0] == '1'; };
  auto is_set = [](const char *name) { return getenv(name) != nullptr; };
  // 0 when unset, otherwise the value clamped to [lo, hi]
  auto number = [](const char *name, long long lo, long long hi) {
    const char *v = getenv(name);
    return v ? (int)std::max(lo, std::min(hi, atoll(v))) : 0;
  };
  Knobs k;
  k.plan.groups = !is_one("BA_NO_GROUPS");
  k.plan.lin_groups = !is_one("BA_NO_LINGRP");
  k.plan.superset = !is_one("BA_NO_SUPERSET");
  k.plan.interleave = !is_one("BA_NO_INTERLEAVE");
  k.plan.split = !is_one("BA_NO_SPLIT");
  k.plan.sup_cap = number("BA_SUP_CAP", 1, 1 << 30);
  k.plan.lin_steps = number("BA_LIN_STEPS", 1, 1 << 30);
  k.plan.threads = number("BA_PLAN_THREADS", 1, 16);
  k.plan.stats = is_set("BA_PLAN_STATS");
  k.plan.times = is_set("BA_PLAN_TIMES");
  k.dense = DenseKnobs::from_env();
  k.cone = ConeKnobs::from_env();
  k.run.force_side = is_one("BA_FORCE_SIDE");
  k.run.overlap = !is_one("BA_NO_OVERLAP");
  k.run.graph = is_one("BA_GRAPH");
  k.run.cost_wide = is_one("BA_COST_WIDE");
  k.run.cov_batch = number("BA_COV_BATCH", 1, 1 << 30);
  k.run.stream_sync = is_one("BA_STREAM_SYNC");
  {
    const char *v = getenv("BA_PAIR_SLIM");
    k.layout.pair_slim = !(v && v[0] == '0');
    const char *o = getenv("BA_PAIR_OBS");
    k.layout.pair_obs = !(o && o[0] == '0');
  }
  return k;
}

}  // namespace ba
#endif
