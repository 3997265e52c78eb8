// Host-only check of the launch plan of the reduced-system solve (csrc/ba_dense_sched.cpp:
// dense_launch_plan, dense_flow_order, dense_dag_items, dense_pick_tile_order): which forward
// sweep, tail kernel and backward sweep run for a schedule under each BA_DENSE_* setting.
//
// Every case prints one line with all fields of its plan; the lines must equal
// dense_launch_expected.txt (argv[1]).  That table was NOT written by the code under test: the
// decision expressions of the launch macro this plan replaced (the tail levels, `split`,
// `flow`, `flow_back`, `dag`, `look2_fits`, `look2`, the list builders and the tile-order pick
// as they stood inline in dense_factor_solve / ba_finalize) were lifted verbatim into a
// stand-alone program that ran over the same cases.  Beside the table the check asserts the
// invariants the launch code relies on, and that the cases reach every path.
// Compiled with g++ by tests/test_plan_invariants.py.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "ba_dense_sched.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (g_fail < 20) {                                  \
        std::printf("FAIL line %d: ", __LINE__);          \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                                \
      }                                                   \
      ++g_fail;                                           \
    }                                                     \
  } while (0)

struct Setting {
  const char *name;
  ba::DenseKnobs knobs;
  bool flow_allowed;  // false: a captured graph is in use
  bool no_tail;       // the no-tail variant (ba_covariance) of the plan the lists were built for
};

static std::vector<Setting> settings() {
  std::vector<Setting> v;
  auto add = [&](const char *name, void (*edit)(ba::DenseKnobs &), bool flow_allowed = true, bool no_tail = false) {
    Setting s{name, ba::DenseKnobs(), flow_allowed, no_tail};
    edit(s.knobs);
    v.push_back(s);
  };
  add("default", [](ba::DenseKnobs &) {});
  add("SPLIT=1", [](ba::DenseKnobs &k) { k.want_split = true; });
  add("TAIL=0", [](ba::DenseKnobs &k) { k.want_tail = false; });
  add("FLOW=0", [](ba::DenseKnobs &k) { k.want_flow = false; });
  add("DAG=0", [](ba::DenseKnobs &k) { k.want_dag = false; });
  add("DAG=1", [](ba::DenseKnobs &k) { k.force_dag = true; });
  add("LOOK2=0", [](ba::DenseKnobs &k) { k.want_look2 = false; });
  add("LOOK2=1", [](ba::DenseKnobs &k) { k.force_look2 = true; });
  add("DAG=0,LOOK2=0", [](ba::DenseKnobs &k) { k.want_dag = k.want_look2 = false; });
  add("TICKET=1", [](ba::DenseKnobs &k) { k.force_ticket = true; });
  add("no-dataflow", [](ba::DenseKnobs &) {}, false);
  add("no-tail-variant", [](ba::DenseKnobs &) {}, true, true);
  return v;
}

struct Row {  // what one line of the table shows
  ba::DenseLaunchPlan plan;
  size_t n_order = 0, n_items = 0;  // lengths of the uploaded flow order and DAG item list
};

static Row plan_row(const ba::DenseSchedule &sc, const Setting &st) {
  Row r;
  // the lists are built for the plan of the upload; the no-tail variant is derived from it afterwards
  const ba::DenseLaunchPlan uploaded = ba::dense_launch_plan(sc, st.knobs, st.flow_allowed);
  r.plan = st.no_tail ? ba::dense_launch_plan_no_tail(sc, st.knobs, st.flow_allowed, uploaded) : uploaded;
  std::vector<int> order, items, pre, need, ntrsm, lneed;
  ba::dense_flow_order(sc, uploaded, order);
  if (uploaded.n_dag_items > 0) ba::dense_dag_items(sc, uploaded, items, pre, need, ntrsm, lneed);
  r.n_order = order.size();
  r.n_items = items.size() / 2;
  CHECK((int)r.n_items == uploaded.n_dag_items, "n_dag_items %d but %zu items built", uploaded.n_dag_items, r.n_items);
  return r;
}

static std::string format_row(const std::string &name, const ba::DenseSchedule &sc, const Setting &st, const Row &r) {
  const ba::DenseLaunchPlan &p = r.plan;
  char buf[512];
  std::snprintf(buf, sizeof buf,
                "%s nb=%d n=%d levels=%d max_rows=%d %s: split=%d tail_levels=%d tail_cols=%d tail_c0=%d pair=%d "
                "back_t_end=%d n_dag_items=%d fwd=%s back=%s ticket=%d order=%zu items=%zu",
                name.c_str(), sc.nb, sc.ncb, sc.nlev, sc.max_rows, st.name, (int)p.split, p.tail_levels, p.tail_cols,
                p.tail_c0, (int)p.tail_pair, p.back_t_end, p.n_dag_items, ba::dense_fwd_name(p.fwd),
                ba::dense_back_name(p.back), (int)p.force_ticket, r.n_order, r.n_items);
  return buf;
}

static std::set<std::string> g_fwd, g_back, g_tail;

static void check_invariants(const std::string &line, const ba::DenseSchedule &sc, const Setting &st, const Row &r) {
  const ba::DenseLaunchPlan &p = r.plan;
  const bool fwd_per_level = p.fwd == ba::DenseFwd::kSplit || p.fwd == ba::DenseFwd::kDiagTrsm;
  // (k_chol_dag and k_chol_look exclude each other by construction: one enum value)
  if (p.fwd == ba::DenseFwd::kDag || p.fwd == ba::DenseFwd::kLook)
    CHECK(p.split && st.flow_allowed && st.knobs.want_flow && p.n_dag_items > 0, "%s: lookahead without its conditions", line.c_str());
  if (!st.no_tail) CHECK((int)r.n_order == p.back_t_end, "%s: the flow order does not cover [0, back_t_end)", line.c_str());
  if (!st.flow_allowed || !st.knobs.want_flow)
    CHECK(fwd_per_level && p.back == ba::DenseBack::kPerLevel, "%s: a dataflow launch although not allowed", line.c_str());
  if (st.no_tail) {
    CHECK(p.tail_levels == 0 && p.tail_cols == 0, "%s: the no-tail variant has a tail", line.c_str());
    if ((int)r.n_order != p.back_t_end)  // the lists were built for a tail
      CHECK(fwd_per_level && p.back == ba::DenseBack::kPerLevel, "%s: dataflow launch on lists of another tail", line.c_str());
  }
  CHECK(p.tail_levels == 0 || (p.tail_levels >= 2 && (p.tail_cols == 64 || p.tail_cols == 96)), "%s: tail form", line.c_str());
  CHECK(p.back_t_end == sc.lev_ptr[sc.nlev - p.tail_levels] && p.tail_c0 == (p.tail_levels ? p.back_t_end * sc.nb : 0),
        "%s: tail position", line.c_str());
  // two levels of 64-column tiles already exceed kTailCols: no tail at tile order 64
  CHECK(sc.nb == 32 || p.tail_levels == 0, "%s: tail at tile order 64", line.c_str());
  g_fwd.insert(ba::dense_fwd_name(p.fwd));
  g_back.insert(ba::dense_back_name(p.back));
  g_tail.insert(p.tail_levels == 0 ? "none" : std::to_string(p.tail_cols) + (p.tail_pair ? " paired" : ""));
}

static std::vector<std::string> g_lines;

static void run(const std::string &name, int n, const std::vector<uint8_t> &adj, int nb) {
  ba::DenseSchedule sc;
  ba::build_dense_schedule(n, adj, false, nb, sc);
  for (const Setting &st : settings()) {
    const Row r = plan_row(sc, st);
    const std::string line = format_row(name, sc, st, r);
    check_invariants(line, sc, st, r);
    g_lines.push_back(line);
  }
}

static void pick(int nlev32, int max_rows32, int nlev64, int force_nb) {
  ba::DenseSchedule s32, s64;
  s32.nb = 32, s32.nlev = nlev32, s32.max_rows = max_rows32;
  s64.nb = 64, s64.nlev = nlev64;
  char buf[160];
  std::snprintf(buf, sizeof buf, "pick nlev32=%d max_rows32=%d nlev64=%d force=%d -> nb%d", nlev32, max_rows32, nlev64,
                force_nb, ba::dense_pick_tile_order(s32, s64, force_nb) == 0 ? 32 : 64);
  g_lines.push_back(buf);
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: dense_launch_check dense_launch_expected.txt\n");
    return 2;
  }
  std::mt19937 gen(5);
  for (int nb : {32, 64})
    for (int n : {4, 7, 12, 24, 40}) {
      for (int band : {1, 3}) {
        std::vector<uint8_t> adj((size_t)n * n, 0);
        for (int i = 0; i < n; ++i)
          for (int j = 0; j < n; ++j)
            if (i != j && std::abs(i - j) <= band) adj[(size_t)i * n + j] = 1;
        run("band" + std::to_string(band), n, adj, nb);
      }
      {
        std::vector<uint8_t> adj((size_t)n * n, 1);
        for (int i = 0; i < n; ++i) adj[(size_t)i * n + i] = 0;
        run("dense", n, adj, nb);
      }
      {  // chain + random closures
        std::vector<uint8_t> adj((size_t)n * n, 0);
        for (int i = 0; i + 1 < n; ++i) adj[(size_t)i * n + i + 1] = adj[(size_t)(i + 1) * n + i] = 1;
        for (int k = 0; k < n; ++k) {
          const int i = gen() % n, j = gen() % n;
          if (i != j) adj[(size_t)i * n + j] = adj[(size_t)j * n + i] = 1;
        }
        run("random", n, adj, nb);
      }
      {  // two chains and an isolated tile between them
        const int h = n / 2;
        std::vector<uint8_t> adj((size_t)n * n, 0);
        for (int i = 0; i + 1 < h - 1; ++i) adj[(size_t)i * n + i + 1] = adj[(size_t)(i + 1) * n + i] = 1;
        for (int i = h; i + 1 < n; ++i) adj[(size_t)i * n + i + 1] = adj[(size_t)(i + 1) * n + i] = 1;
        run("disconnected", n, adj, nb);
      }
    }
  {  // dense and large enough for more than kDagMaxItems items: k_chol_look by default
    const int n = 48;
    std::vector<uint8_t> adj((size_t)n * n, 1);
    for (int i = 0; i < n; ++i) adj[(size_t)i * n + i] = 0;
    run("dense", n, adj, 64);
  }
  // tile-order pick: narrow rule (max_rows <= 6), chain cost (16 us x levels at 32 against 30 us at 64), overrides
  pick(8, 4, 8, 0);     // narrow, nb32 cheaper
  pick(10, 6, 5, 0);    // narrow, nb64 cheaper (160 against 150)
  pick(15, 6, 8, 0);    // narrow, equal cost: nb32
  pick(8, 7, 8, 0);     // not narrow: nb64 whatever the cost
  pick(8, 7, 8, 32);    // override to 32
  pick(8, 4, 8, 64);    // override to 64
  pick(8, 4, 8, 16);    // any other value: no override
  pick(10, 6, 5, 32);

  // the cases reach every path the replaced logic could produce (tail at tile order 64: see above)
  CHECK(g_fwd.size() == 5, "forward sweeps reached: %zu of 5", g_fwd.size());
  CHECK(g_back.size() == 3, "backward sweeps reached: %zu of 3", g_back.size());
  for (const char *t : {"none", "64", "96", "96 paired"}) CHECK(g_tail.count(t), "tail form '%s' not reached", t);

  std::vector<std::string> expected;
  std::ifstream in(argv[1]);
  for (std::string l; std::getline(in, l);)
    if (!l.empty() && l[0] != '#') expected.push_back(l);
  CHECK(expected.size() == g_lines.size(), "%zu cases, %zu expected lines", g_lines.size(), expected.size());
  for (size_t k = 0; k < g_lines.size(); ++k) {
    std::printf("%s\n", g_lines[k].c_str());
    if (k < expected.size()) CHECK(g_lines[k] == expected[k], "expected: %s\n          got: %s", expected[k].c_str(), g_lines[k].c_str());
  }
  std::printf(g_fail ? "DENSE LAUNCH CHECK FAILED (%d)\n" : "DENSE LAUNCH CHECK OK\n", g_fail);
  return g_fail ? 1 : 0;
}
