// Host-only check of the knob record (csrc/ba_knobs.h), compiled with g++ by
// tests/test_plan_invariants.py.  In ONE process: with no BA_* variable set,
// Knobs::from_env() is the default-constructed record; each variable in turn, set to a
// non-default value, changes exactly its field; unset again, the default is back (a value
// cached on first use would fail the second and third step).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "ba_knobs.h"

extern char **environ;

static int g_fail = 0;

// Every field by name.  The structured bindings name ALL members of each struct: a new
// field does not compile until it is listed here (and gets a case below).
static std::vector<std::pair<const char *, long>> fields(const ba::Knobs &k) {
  const auto &[groups, lin_groups, superset, interleave, split, sup_cap, lin_steps, threads, stats, times] = k.plan;
  const auto &[want_split, want_tail, want_flow, want_dag, force_dag, want_look2, force_look2, force_ticket, natural, full,
               nb, order] = k.dense;
  const auto &[force_side, overlap, graph, cost_wide, cov_batch, stream_sync] = k.run;
  return {{"plan.groups", groups}, {"plan.lin_groups", lin_groups}, {"plan.superset", superset},
          {"plan.interleave", interleave}, {"plan.split", split}, {"plan.sup_cap", sup_cap},
          {"plan.lin_steps", lin_steps}, {"plan.threads", threads}, {"plan.stats", stats}, {"plan.times", times},
          {"dense.want_split", want_split}, {"dense.want_tail", want_tail}, {"dense.want_flow", want_flow},
          {"dense.want_dag", want_dag}, {"dense.force_dag", force_dag}, {"dense.want_look2", want_look2},
          {"dense.force_look2", force_look2}, {"dense.force_ticket", force_ticket}, {"dense.natural", natural},
          {"dense.full", full}, {"dense.nb", nb}, {"dense.order", order},
          {"run.force_side", force_side}, {"run.overlap", overlap}, {"run.graph", graph},
          {"run.cost_wide", cost_wide}, {"run.cov_batch", cov_batch}, {"run.stream_sync", stream_sync}};
}

static void expect_equal(const ba::Knobs &got, const ba::Knobs &want, const std::string &what) {
  const auto g = fields(got), w = fields(want);
  for (size_t i = 0; i < g.size(); ++i)
    if (g[i].second != w[i].second) {
      std::printf("FAIL %s: %s = %ld, expected %ld\n", what.c_str(), g[i].first, g[i].second, w[i].second);
      ++g_fail;
    }
}

struct Case {
  const char *name, *value;
  void (*edit)(ba::Knobs &);  // what the setting does to the default record
};

int main() {
  std::vector<std::string> set_before;
  for (char **e = environ; *e; ++e)
    if (!std::strncmp(*e, "BA_", 3)) set_before.push_back(std::string(*e, std::strcspn(*e, "=")));
  for (const std::string &n : set_before) unsetenv(n.c_str());

  const ba::Knobs def;
  expect_equal(ba::Knobs::from_env(), def, "clean environment");

  const Case cases[] = {
      {"BA_NO_GROUPS", "1", [](ba::Knobs &k) { k.plan.groups = false; }},
      {"BA_NO_LINGRP", "1", [](ba::Knobs &k) { k.plan.lin_groups = false; }},
      {"BA_NO_SUPERSET", "1", [](ba::Knobs &k) { k.plan.superset = false; }},
      {"BA_NO_INTERLEAVE", "1", [](ba::Knobs &k) { k.plan.interleave = false; }},
      {"BA_NO_SPLIT", "1", [](ba::Knobs &k) { k.plan.split = false; }},
      {"BA_SUP_CAP", "7", [](ba::Knobs &k) { k.plan.sup_cap = 7; }},
      {"BA_SUP_CAP", "-3", [](ba::Knobs &k) { k.plan.sup_cap = 1; }},
      {"BA_LIN_STEPS", "2", [](ba::Knobs &k) { k.plan.lin_steps = 2; }},
      {"BA_PLAN_THREADS", "7", [](ba::Knobs &k) { k.plan.threads = 7; }},
      {"BA_PLAN_THREADS", "0", [](ba::Knobs &k) { k.plan.threads = 1; }},
      {"BA_PLAN_THREADS", "99", [](ba::Knobs &k) { k.plan.threads = 16; }},
      {"BA_PLAN_STATS", "1", [](ba::Knobs &k) { k.plan.stats = true; }},
      {"BA_PLAN_TIMES", "1", [](ba::Knobs &k) { k.plan.times = true; }},
      {"BA_DENSE_SPLIT", "1", [](ba::Knobs &k) { k.dense.want_split = true; }},
      {"BA_DENSE_TAIL", "0", [](ba::Knobs &k) { k.dense.want_tail = false; }},
      {"BA_DENSE_FLOW", "0", [](ba::Knobs &k) { k.dense.want_flow = false; }},
      {"BA_DENSE_DAG", "0", [](ba::Knobs &k) { k.dense.want_dag = false; }},
      {"BA_DENSE_DAG", "1", [](ba::Knobs &k) { k.dense.force_dag = true; }},
      {"BA_DENSE_LOOK2", "0", [](ba::Knobs &k) { k.dense.want_look2 = false; }},
      {"BA_DENSE_LOOK2", "1", [](ba::Knobs &k) { k.dense.force_look2 = true; }},
      {"BA_DENSE_TICKET", "1", [](ba::Knobs &k) { k.dense.force_ticket = true; }},
      {"BA_DENSE_NATURAL", "1", [](ba::Knobs &k) { k.dense.natural = true; }},
      {"BA_DENSE_FULL", "1", [](ba::Knobs &k) { k.dense.full = true; }},
      {"BA_DENSE_NB", "64", [](ba::Knobs &k) { k.dense.nb = 64; }},
      {"BA_DENSE_ORDER", "strict", [](ba::Knobs &k) { k.dense.order = 's'; }},
      {"BA_DENSE_ORDER", "relaxed", [](ba::Knobs &k) { k.dense.order = 'r'; }},
      {"BA_FORCE_SIDE", "1", [](ba::Knobs &k) { k.run.force_side = true; }},
      {"BA_NO_OVERLAP", "1", [](ba::Knobs &k) { k.run.overlap = false; }},
      {"BA_GRAPH", "1", [](ba::Knobs &k) { k.run.graph = true; }},
      {"BA_COST_WIDE", "1", [](ba::Knobs &k) { k.run.cost_wide = true; }},
      {"BA_COV_BATCH", "64", [](ba::Knobs &k) { k.run.cov_batch = 64; }},
      {"BA_STREAM_SYNC", "1", [](ba::Knobs &k) { k.run.stream_sync = true; }},
  };
  for (const Case &c : cases) {
    const std::string what = std::string(c.name) + "=" + c.value;
    ba::Knobs want;
    c.edit(want);
    if (fields(want) == fields(def)) {
      std::printf("FAIL %s: the case expects no change\n", what.c_str());
      ++g_fail;
    }
    setenv(c.name, c.value, 1);
    expect_equal(ba::Knobs::from_env(), want, what);
    unsetenv(c.name);
    expect_equal(ba::Knobs::from_env(), def, what + ", then unset");
  }
  // every field of the record is reached by at least one case
  {
    std::vector<int> hit(fields(def).size(), 0);
    for (const Case &c : cases) {
      ba::Knobs want;
      c.edit(want);
      const auto w = fields(want), d = fields(def);
      for (size_t i = 0; i < w.size(); ++i) hit[i] |= w[i].second != d[i].second;
    }
    const auto d = fields(def);
    for (size_t i = 0; i < d.size(); ++i)
      if (!hit[i]) {
        std::printf("FAIL no case changes %s\n", d[i].first);
        ++g_fail;
      }
  }
  if (g_fail) return 1;
  std::printf("KNOBS CHECK OK (%zu settings, %zu fields)\n", sizeof(cases) / sizeof(cases[0]), fields(def).size());
  return 0;
}
