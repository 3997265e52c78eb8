// Host-only check of the cone sweep's lists (csrc/ba_dense_sched.cpp: dense_cone_lists and
// the back_cone decision of dense_launch_plan), the backward sweep in which the workgroup of
// a leaf solves its own chain of ancestors (k_chol_back_cone).
//
// For chains of 1 .. 199 tiles, bands of 2 .. 4, an arrow, a dense 6-tile pattern and two
// disconnected chains, at tile orders 32 and 64, with and without a tail (and, for the caps, a
// chain in natural order, whose single cone is the whole chain, a broom, whose cones all run
// through the same ancestors, and a dense 24-tile pattern), the check recomputes leaves and cones from their
// definition — plain set closure over rows[], nothing shared with the code under test — and
// asserts that
//   - the leaves are exactly the non-tail positions that are no row tile of another one;
//   - every cone is closed under rows[], in strictly descending position, the leaf last;
//   - every row-tile reference names the position rows[] names and a slot that is an EARLIER
//     step of the same cone holding that position, or the tail tile's own slot;
//   - every non-tail position is stored by exactly one leaf, the lowest whose cone holds it;
//   - BA_DENSE_CONE is read anew at every ConeKnobs::from_env;
//   - the path is selected exactly when the knob, the tail of the lists, kBackGatherMaxRows,
//     kConeMaxLen and kConeMaxWork say so, and `back` and every other field of the plan do
//     not depend on it;
//   - the 199-tile chain has the pinned number of leaves and longest cone.
// Compiled with g++ by tests/test_dense_cone.py (once more with -fsanitize=address,undefined).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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

static std::set<std::string> g_outcomes;  // which decisions the cases reach

// Row tiles of position q (without the rhs block).
static std::vector<int> rows_of(const ba::DenseSchedule &sc, int q) {
  std::vector<int> r;
  for (int a = sc.row_ptr[q]; a < sc.row_ptr[q + 1]; ++a)
    if (sc.rows[a] < sc.ncb) r.push_back(sc.rows[a]);
  return r;
}

struct Expect {
  std::vector<int> leaves;
  std::vector<std::set<int>> cones;  // non-tail ancestors and the leaf itself
  int max_len = 0;
  long steps = 0;
};

static Expect expect(const ba::DenseSchedule &sc, int t_end) {
  Expect e;
  std::set<int> is_row;
  for (int q = 0; q < t_end; ++q)
    for (int I : rows_of(sc, q))
      if (I < t_end) is_row.insert(I);
  for (int p = 0; p < t_end; ++p) {
    if (is_row.count(p)) continue;
    std::set<int> cone{p};
    for (bool grown = true; grown;) {  // closure by repeated passes
      grown = false;
      for (int q : std::vector<int>(cone.begin(), cone.end()))
        for (int I : rows_of(sc, q))
          if (I < t_end && cone.insert(I).second) grown = true;
    }
    e.leaves.push_back(p);
    e.max_len = std::max(e.max_len, (int)cone.size());
    e.steps += (long)cone.size();
    e.cones.push_back(cone);
  }
  return e;
}

static void check_lists(const std::string &name, const ba::DenseSchedule &sc, const ba::DenseLaunchPlan &pl,
                        const Expect &e) {
  ba::DenseCone cone;
  ba::dense_cone_lists(sc, pl, cone);
  const int T = pl.back_t_end, stride = pl.cone_max;
  CHECK(cone.leaf == e.leaves, "%s: leaves", name.c_str());
  CHECK(pl.cone_leaves == (int)e.leaves.size() && pl.cone_max == e.max_len && pl.cone_steps == e.steps,
        "%s: plan says %d leaves, longest %d, %d steps; expected %zu, %d, %ld", name.c_str(), pl.cone_leaves, pl.cone_max,
        pl.cone_steps, e.leaves.size(), e.max_len, e.steps);
  CHECK(cone.rec.size() == cone.leaf.size() * (size_t)stride * ba::kConeRec, "%s: record array size", name.c_str());
  if (cone.leaf != e.leaves || cone.rec.size() != cone.leaf.size() * (size_t)stride * ba::kConeRec) return;
  std::vector<int> stores((size_t)T, 0), first_leaf((size_t)T, -1);
  for (size_t lf = 0; lf < cone.leaf.size(); ++lf) {
    const int len = cone.len[lf];
    CHECK(len == (int)e.cones[lf].size() && len >= 1 && len <= stride, "%s leaf %zu: %d steps", name.c_str(), lf, len);
    std::vector<int> pos;
    for (int k = 0; k < len; ++k) {
      const int *r = &cone.rec[(lf * stride + k) * ba::kConeRec];
      const int q = r[0];
      pos.push_back(q);
      CHECK(q >= 0 && q < T && e.cones[lf].count(q), "%s leaf %zu step %d: position %d not in the cone", name.c_str(), lf, k, q);
      CHECK(k == 0 || q < pos[k - 1], "%s leaf %zu step %d: not descending", name.c_str(), lf, k);
      CHECK(r[3] == len, "%s leaf %zu step %d: step count", name.c_str(), lf, k);
      if (q < 0 || q >= T) continue;
      const std::vector<int> rows = rows_of(sc, q);
      CHECK(r[1] == (int)rows.size() && r[1] <= ba::kBackGatherMaxRows - 1, "%s leaf %zu step %d: nrow %d", name.c_str(), lf, k, r[1]);
      for (int a = 0; a < ba::kBackGatherMaxRows - 1; ++a) {
        const int I = r[4 + a] & ((1 << ba::kConeSlotShift) - 1), slot = r[4 + a] >> ba::kConeSlotShift;
        if (a < (int)rows.size()) {
          CHECK(I == rows[a], "%s leaf %zu step %d row %d: tile %d, rows[] has %d", name.c_str(), lf, k, a, I, rows[a]);
          if (I >= T) {
            CHECK(I < sc.ncb && slot == I - T && slot < ba::kConeTailSlots, "%s leaf %zu step %d row %d: tail slot %d", name.c_str(), lf, k, a, slot);
          } else {
            const int step = slot - ba::kConeTailSlots;  // closure: it is a step; order: an earlier one
            CHECK(step >= 0 && step < k && pos[step] == I, "%s leaf %zu step %d row %d: slot %d does not hold tile %d", name.c_str(), lf, k, a, slot, I);
          }
        } else {  // padding: any readable tile and slot (its product is not used)
          CHECK(I >= 0 && I < sc.ncb && slot >= 0 && slot <= ba::kConeTailSlots + k, "%s leaf %zu step %d: padding", name.c_str(), lf, k);
        }
      }
      CHECK(r[2] == 0 || r[2] == 1, "%s: store flag", name.c_str());
      stores[q] += r[2];
      if (first_leaf[q] < 0) first_leaf[q] = (int)lf;
      CHECK(r[2] == (first_leaf[q] == (int)lf ? 1 : 0), "%s leaf %zu step %d: not the lowest leaf's store", name.c_str(), lf, k);
    }
    CHECK(!pos.empty() && pos.back() == cone.leaf[lf], "%s leaf %zu: the leaf is not the last step", name.c_str(), lf);
  }
  for (int q = 0; q < T; ++q) {
    CHECK(stores[q] == 1, "%s: position %d stored by %d leaves", name.c_str(), q, stores[q]);
    CHECK(cone.writer[q] == first_leaf[q], "%s: writer of %d", name.c_str(), q);
  }
}

static void run(const std::string &pattern, int n, const std::vector<uint8_t> &adj, int nb, bool natural = false) {
  ba::DenseSchedule sc;
  ba::build_dense_schedule(n, adj, natural, nb, sc);
  for (int tail = 0; tail < 2; ++tail) {
    ba::DenseKnobs knobs;
    knobs.want_tail = tail != 0;
    const std::string name = pattern + std::to_string(n) + " nb" + std::to_string(nb) + (tail ? " tail" : " no-tail");
    const ba::DenseLaunchPlan pl = ba::dense_launch_plan(sc, knobs, true);
    const Expect e = expect(sc, pl.back_t_end);
    const bool want = pl.back_t_end > 0 && sc.max_rows <= ba::kBackGatherMaxRows && e.max_len <= ba::kConeMaxLen &&
                      (double)e.steps <= ba::kConeMaxWork * pl.back_t_end;
    CHECK(pl.back_cone == want, "%s: back_cone %d, the caps say %d (longest %d, %ld steps on %d tiles, max_rows %d)",
          name.c_str(), (int)pl.back_cone, (int)want, e.max_len, e.steps, pl.back_t_end, sc.max_rows);
    g_outcomes.insert(want ? "taken" : pl.back_t_end == 0 ? "empty" : sc.max_rows > ba::kBackGatherMaxRows ? "rows"
                      : e.max_len > ba::kConeMaxLen ? "length" : "work");
    std::printf("%s: levels=%d max_rows=%d tiles=%d leaves=%zu longest=%d steps=%ld cone=%d\n", name.c_str(), sc.nlev,
                sc.max_rows, pl.back_t_end, e.leaves.size(), e.max_len, e.steps, (int)pl.back_cone);
    // the same under "no dataflow" (a captured graph); never on lists of another tail or against the knob
    const ba::DenseLaunchPlan graph = ba::dense_launch_plan(sc, knobs, false);
    CHECK(graph.back_cone == want && graph.cone_leaves == pl.cone_leaves && graph.cone_max == pl.cone_max,
          "%s: the decision depends on flow_allowed", name.c_str());
    CHECK(!ba::dense_launch_plan(sc, knobs, true, /*lists_fit=*/false).back_cone, "%s: cone sweep on lists of another tail", name.c_str());
    const ba::DenseLaunchPlan no_tail = ba::dense_launch_plan_no_tail(sc, knobs, true, pl);
    if (pl.tail_levels > 0) CHECK(!no_tail.back_cone, "%s: the no-tail variant takes lists built for a tail", name.c_str());
    else CHECK(no_tail.back_cone == want, "%s: the no-tail variant of a plan without tail", name.c_str());
    const ba::DenseLaunchPlan po = ba::dense_launch_plan(sc, knobs, true, /*lists_fit=*/true, /*cone_allowed=*/false);
    CHECK(!ba::dense_launch_plan_no_tail(sc, knobs, true, pl, /*cone_allowed=*/false).back_cone, "%s: no-tail variant against the knob", name.c_str());
    CHECK(!po.back_cone && po.cone_leaves == 0, "%s: cone sweep against the knob", name.c_str());
    CHECK(po.back == pl.back && po.fwd == pl.fwd && po.back_t_end == pl.back_t_end && po.tail_levels == pl.tail_levels &&
          po.tail_cols == pl.tail_cols && po.split == pl.split && po.n_dag_items == pl.n_dag_items,
          "%s: another field of the plan depends on the knob", name.c_str());
    if (pl.back_cone) check_lists(name, sc, pl, e);
    if (pattern == "chain" && n == 199 && nb == 32 && tail) {
      // pinned: odd-even reduction of 199 tiles has the levels 100 50 25 12 6 3 | 2 1 (tail)
      CHECK(e.leaves.size() == 100 && e.max_len == 6 && e.steps == 572,
            "chain199: %zu leaves, longest cone %d, %ld steps", e.leaves.size(), e.max_len, e.steps);
    }
  }
}

static std::vector<uint8_t> band(int n, int w) {
  std::vector<uint8_t> adj((size_t)n * n, 0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      if (i != j && std::abs(i - j) <= w) adj[(size_t)i * n + j] = 1;
  return adj;
}

// BA_DENSE_CONE in one process: unset and any value but "0..." allow the sweep, the value is read anew every time.
static void check_knob() {
  unsetenv("BA_DENSE_CONE");
  CHECK(ba::ConeKnobs().want && ba::ConeKnobs::from_env().want, "default: allowed");
  setenv("BA_DENSE_CONE", "0", 1);
  CHECK(!ba::ConeKnobs::from_env().want, "BA_DENSE_CONE=0 forbids");
  setenv("BA_DENSE_CONE", "1", 1);
  CHECK(ba::ConeKnobs::from_env().want, "BA_DENSE_CONE=1 allows");
  unsetenv("BA_DENSE_CONE");
  CHECK(ba::ConeKnobs::from_env().want, "unset again: allowed (no cached value)");
}

int main() {
  check_knob();
  for (int nb : {32, 64}) {
    for (int n : {1, 2, 3, 4, 5, 8, 9, 16, 17, 40, 199}) run("chain", n, band(n, 1), nb);
    for (int n : {12, 40}) run("band3_", n, band(n, 3), nb);
    run("band2_", 80, band(80, 2), nb);
    run("band3_", 120, band(120, 3), nb);
    run("band4_", 60, band(60, 4), nb);
    {  // arrow: every tile coupled to the last
      const int n = 12;
      std::vector<uint8_t> adj((size_t)n * n, 0);
      for (int i = 0; i + 1 < n; ++i) adj[(size_t)i * n + n - 1] = adj[(size_t)(n - 1) * n + i] = 1;
      run("arrow", n, adj, nb);
    }
    run("dense", 6, band(6, 6), nb);
    {  // two disconnected chains
      const int n = 20, h = 9;
      std::vector<uint8_t> adj((size_t)n * n, 0);
      for (int i = 0; i + 1 < n; ++i)
        if (i + 1 != h) adj[(size_t)i * n + i + 1] = adj[(size_t)(i + 1) * n + i] = 1;
      run("two_chains", n, adj, nb);
    }
    {  // a broom: 200 tiles coupled to the first tile of a 60-tile chain — short cones, all through the same ancestors
      const int n = 260, h = 200;
      std::vector<uint8_t> adj((size_t)n * n, 0);
      for (int i = 0; i < h; ++i) adj[(size_t)i * n + h] = adj[(size_t)h * n + i] = 1;
      for (int i = h; i + 1 < n; ++i) adj[(size_t)i * n + i + 1] = adj[(size_t)(i + 1) * n + i] = 1;
      run("broom", n, adj, nb);
    }
    run("natural_chain", 40, band(40, 1), nb, /*natural=*/true);  // one cone of every tile: too long
    run("dense", 24, band(24, 24), nb);                            // too many row tiles per column
  }
  for (const char *o : {"taken", "empty", "rows", "length", "work"}) CHECK(g_outcomes.count(o), "no case reaches the outcome '%s'", o);
  std::printf(g_fail ? "DENSE CONE CHECK FAILED (%d)\n" : "DENSE CONE CHECK OK\n", g_fail);
  return g_fail ? 1 : 0;
}
