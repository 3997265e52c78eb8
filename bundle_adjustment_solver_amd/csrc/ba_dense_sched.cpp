// ba_dense_sched.cpp — see ba_dense_sched.h.  Host-only.
#include "ba_dense_sched.h"

#include <cstdlib>

#include <algorithm>
#include <tuple>

namespace ba {

namespace {

// One schedule.  `relaxed`: tiles of up to about twice the minimum degree may
// enter a level, instead of only the (nearly) minimum-degree ones.  For a block
// tridiagonal pattern both give odd-even cyclic reduction; for wider bands the
// strict rule only ever finds the two ends of the band (n/2 levels), the
// relaxed one eliminates every (band+1)-th tile at once (O(log n) levels, about
// twice the fill).
void build_one(int ncb, const std::vector<uint8_t> &adj_in, bool natural_order, int nb,
               bool relaxed, DenseSchedule &s) {
  const int n = ncb;
  s = DenseSchedule();
  s.nb = nb;
  s.ncb = n;
  std::vector<uint8_t> A(adj_in);
  auto at = [&](int a, int b) -> uint8_t & { return A[(size_t)a * n + b]; };
  for (int v = 0; v < n; ++v) at(v, v) = 0;
  std::vector<uint8_t> alive(n, 1), blocked(n, 0);
  std::vector<int> deg(n, 0);
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b)
      if (a != b && (at(a, b) || at(b, a))) {
        at(a, b) = at(b, a) = 1;
      }
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) deg[a] += at(a, b);
  std::vector<std::vector<int>> rows_of(n);
  s.pos_of_tile.assign(n, -1);
  s.tile_at_pos.clear();
  s.lev_ptr.assign(1, 0);
  int remaining = n, next = 0;
  std::vector<int> cand, level, nv;
  while (remaining > 0) {
    level.clear();
    if (natural_order) {
      for (int v = 0; v < n; ++v)
        if (alive[v]) {
          level.push_back(v);
          break;
        }
    } else {
      int mind = n + 1;
      for (int v = 0; v < n; ++v)
        if (alive[v]) mind = std::min(mind, deg[v]);
      const int thr = relaxed ? 2 * mind + 1 : mind + std::max(1, mind / 4);
      cand.clear();
      for (int v = 0; v < n; ++v)
        if (alive[v] && deg[v] <= thr) cand.push_back(v);
      std::stable_sort(cand.begin(), cand.end(),
                       [&](int a, int b) { return deg[a] < deg[b]; });
      std::fill(blocked.begin(), blocked.end(), 0);
      for (int v : cand) {
        if (blocked[v]) continue;
        level.push_back(v);
        blocked[v] = 1;
        for (int u = 0; u < n; ++u)
          if (alive[u] && at(v, u)) blocked[u] = 1;
      }
      std::sort(level.begin(), level.end());
    }
    // eliminate the independent set: neighbours become cliques (fill-in)
    for (int v : level) {
      nv.clear();
      for (int u = 0; u < n; ++u)
        if (alive[u] && u != v && at(v, u)) nv.push_back(u);
      rows_of[v] = nv;
      for (size_t a = 0; a < nv.size(); ++a)
        for (size_t b = a + 1; b < nv.size(); ++b)
          if (!at(nv[a], nv[b])) {
            at(nv[a], nv[b]) = at(nv[b], nv[a]) = 1;
            deg[nv[a]]++;
            deg[nv[b]]++;
          }
    }
    for (int v : level) {
      alive[v] = 0;
      for (int u : rows_of[v]) deg[u]--;
      s.pos_of_tile[v] = next++;
      s.tile_at_pos.push_back(v);
      --remaining;
    }
    s.lev_ptr.push_back(next);
  }
  s.nlev = (int)s.lev_ptr.size() - 1;

  // rows per position (ascending positions, rhs block last)
  s.row_ptr.assign(n + 1, 0);
  s.rows.clear();
  double nz_tiles = n;
  for (int p = 0; p < n; ++p) {
    std::vector<int> r;
    for (int u : rows_of[s.tile_at_pos[p]]) r.push_back(s.pos_of_tile[u]);
    std::sort(r.begin(), r.end());
    nz_tiles += (double)r.size();
    for (int I : r) s.rows.push_back(I);
    s.rows.push_back(n);
    s.row_ptr[p + 1] = (int)s.rows.size();
    const double m = (double)r.size() + 1.0;  // incl. rhs row block
    const double c3 = 64.0 * 64.0 * 64.0;
    s.flops += c3 / 3.0 + m * c3 + m * (m + 1.0) * c3;
  }
  s.fill = nz_tiles / ((double)n * (n + 1) / 2.0);

  // work lists per level
  s.item_ptr.assign(1, 0);
  s.tgt_ptr.assign(1, 0);
  s.tgt_first.clear();
  s.tgt_src_ptr.clear();
  std::vector<std::tuple<int, int, int>> trip;
  for (int l = 0; l < s.nlev; ++l) {
    trip.clear();
    for (int p = s.lev_ptr[l]; p < s.lev_ptr[l + 1]; ++p) {
      const int b = s.row_ptr[p], e = s.row_ptr[p + 1];
      for (int a = b; a < e; ++a) {
        s.item_t.push_back(p);
        s.item_I.push_back(s.rows[a]);
        for (int c = b; c <= a; ++c)
          if (s.rows[c] < n) trip.emplace_back(s.rows[a], s.rows[c], p);
      }
    }
    s.item_ptr.push_back((int)s.item_t.size());
    // target-centric: every (I,J) tile touched in this level, with the panels
    // that update it in ascending position order
    // (targets in a column that is eliminated in the NEXT level come first: with
    //  lookahead — dense patterns — they are updated before the rest, so that the next
    //  level's factorisation can start beside the bulk of this level's update)
    auto next_level = [&](int J) { return l + 1 < s.nlev && J >= s.lev_ptr[l + 1] && J < s.lev_ptr[l + 2]; };
    std::sort(trip.begin(), trip.end(), [&](const std::tuple<int, int, int> &x, const std::tuple<int, int, int> &y) {
      const int nx = next_level(std::get<1>(x)) ? 0 : 1, ny = next_level(std::get<1>(y)) ? 0 : 1;
      if (nx != ny) return nx < ny;
      return x < y;
    });
    int n_first = 0;
    for (size_t k = 0; k < trip.size(); ++k) {
      const bool is_new = k == 0 ||
                          std::get<0>(trip[k]) != std::get<0>(trip[k - 1]) ||
                          std::get<1>(trip[k]) != std::get<1>(trip[k - 1]);
      if (is_new) {
        s.tgt_I.push_back(std::get<0>(trip[k]));
        s.tgt_J.push_back(std::get<1>(trip[k]));
        s.tgt_src_ptr.push_back((int)s.src_t.size());
        n_first += next_level(std::get<1>(trip[k])) ? 1 : 0;
      }
      s.src_t.push_back(std::get<2>(trip[k]));
    }
    s.tgt_first.push_back(n_first);
    s.tgt_ptr.push_back((int)s.tgt_I.size());
  }
  s.tgt_src_ptr.push_back((int)s.src_t.size());
  s.tgt_desc.assign(8 * s.tgt_I.size(), -1);
  for (size_t tg = 0; tg < s.tgt_I.size(); ++tg) {
    int *q = &s.tgt_desc[8 * tg];
    q[0] = s.tgt_I[tg];
    q[1] = s.tgt_J[tg];
    q[2] = s.tgt_src_ptr[tg + 1] - s.tgt_src_ptr[tg];
    q[3] = s.tgt_src_ptr[tg];
    for (int k = 0; k < 4 && k < q[2]; ++k) q[4 + k] = s.src_t[q[3] + k];
  }
  s.row_desc.assign(16 * (size_t)n, -1);
  for (int p = 0; p < n; ++p) {
    int *q = &s.row_desc[16 * (size_t)p];
    q[0] = s.row_ptr[p + 1] - s.row_ptr[p];
    q[1] = s.row_ptr[p];
    s.max_rows = std::max(s.max_rows, q[0]);
    for (int k = 2; k < 8; ++k) q[k] = 0;
    for (int a = 0; a < 8 && a < q[0]; ++a) q[8 + a] = s.rows[q[1] + a];
  }
  s.back_desc.assign(8 * (size_t)n, -1);
  for (int p = 0; p < n; ++p) {
    int *q = &s.back_desc[8 * (size_t)p];
    int cnt = 0;
    for (int a = s.row_ptr[p]; a < s.row_ptr[p + 1] && s.rows[a] < n; ++a) ++cnt;
    q[0] = cnt;
    q[1] = s.row_ptr[p];
    for (int k = 0; k < 6 && k < cnt; ++k) q[2 + k] = s.rows[q[1] + k];
  }
}

// Leaves and cones of the non-tail positions [0, t_end) (see DenseCone): calls
// visit(index of the leaf, cone) per leaf in ascending position, the cone in descending
// position.  Stops and returns false at the first cone of more than max_len steps.
template <class Visit>
bool walk_cones(const DenseSchedule &sc, int t_end, int max_len, Visit visit) {
  std::vector<uint8_t> is_row((size_t)t_end, 0);
  for (int q = 0; q < t_end; ++q)
    for (int a = sc.row_ptr[q]; a < sc.row_ptr[q + 1]; ++a)
      if (sc.rows[a] < t_end) is_row[sc.rows[a]] = 1;
  std::vector<int> seen((size_t)t_end, -1), cone, stack;
  int n_leaf = 0;
  for (int p = 0; p < t_end; ++p) {
    if (is_row[p]) continue;
    cone.clear();
    stack.assign(1, p);
    seen[p] = p;
    while (!stack.empty()) {
      const int q = stack.back();
      stack.pop_back();
      cone.push_back(q);
      if ((int)cone.size() > max_len) return false;
      for (int a = sc.row_ptr[q]; a < sc.row_ptr[q + 1]; ++a) {
        const int I = sc.rows[a];
        if (I < t_end && seen[I] != p) {
          seen[I] = p;
          stack.push_back(I);
        }
      }
    }
    std::sort(cone.begin(), cone.end(), [](int a, int b) { return a > b; });
    visit(n_leaf++, cone);
  }
  return true;
}

}  // namespace

void build_dense_schedule(int ncb, const std::vector<uint8_t> &adj, bool natural_order, int nb,
                          DenseSchedule &s, char order) {
  if (natural_order || order == 's') {
    build_one(ncb, adj, natural_order, nb, false, s);
    return;
  }
  if (order == 'r') {
    build_one(ncb, adj, false, nb, true, s);
    return;
  }
  // the solve is a chain of dependent launches per level whose length grows
  // mildly with the row tiles a column carries: keep the shorter chain
  DenseSchedule relaxed;
  build_one(ncb, adj, false, nb, false, s);
  build_one(ncb, adj, false, nb, true, relaxed);
  auto chain = [](const DenseSchedule &q) { return q.nlev * (1.0 + 0.1 * q.max_rows); };
  if (chain(relaxed) < chain(s)) s = relaxed;
}

DenseKnobs DenseKnobs::from_env() {
  auto value = [](const char *name) { const char *v = getenv(name); return v ? v : ""; };
  auto first = [&](const char *name) { return value(name)[0]; };
  auto number = [&](const char *name) { return atoi(value(name)); };
  DenseKnobs k;
  k.want_split = first("BA_DENSE_SPLIT") == '1';
  k.want_tail = first("BA_DENSE_TAIL") != '0';
  k.want_flow = first("BA_DENSE_FLOW") != '0';
  k.want_dag = first("BA_DENSE_DAG") != '0';
  k.force_dag = first("BA_DENSE_DAG") == '1';
  k.want_look2 = first("BA_DENSE_LOOK2") != '0';
  k.force_look2 = first("BA_DENSE_LOOK2") == '1';
  k.force_ticket = first("BA_DENSE_TICKET") == '1';
  k.natural = number("BA_DENSE_NATURAL") != 0;
  k.full = number("BA_DENSE_FULL") != 0;
  k.nb = number("BA_DENSE_NB");
  const char o = first("BA_DENSE_ORDER");
  k.order = (o == 's' || o == 'r') ? o : '\0';
  return k;
}

ConeKnobs ConeKnobs::from_env() {
  const char *v = getenv("BA_DENSE_CONE");
  ConeKnobs k;
  k.want = !(v && v[0] == '0');
  return k;
}

const char *dense_fwd_name(DenseFwd f) {
  static const char *const names[] = {"look", "dag", "level_flow", "diag_trsm", "split"};
  return names[(int)f];
}
const char *dense_back_name(DenseBack b) {
  static const char *const names[] = {"flow_gather", "flow_ordered", "per_level"};
  return names[(int)b];
}

DenseLaunchPlan dense_launch_plan(const DenseSchedule &sc, const DenseKnobs &knobs, bool flow_allowed,
                                  bool lists_fit, bool cone_allowed) {
  DenseLaunchPlan p;
  p.force_ticket = knobs.force_ticket;
  p.split = knobs.want_split || sc.max_rows > dense_fused_max_rows(sc.nb);
  if (knobs.want_tail) {
    for (int l = sc.nlev - 1; l >= 0; --l) {
      const int cols = (sc.lev_ptr[l + 1] - sc.lev_ptr[l]) * sc.nb;
      if (p.tail_cols + cols > kTailCols) break;
      p.tail_cols += cols;
      ++p.tail_levels;
    }
    if (p.tail_levels < 2 || (p.tail_cols != 64 && p.tail_cols != 96)) p.tail_levels = p.tail_cols = 0;
  }
  const int nlv = sc.nlev - p.tail_levels;  // levels of the sweeps
  p.back_t_end = sc.lev_ptr[nlv];
  if (p.tail_levels > 0) {
    p.tail_c0 = p.back_t_end * sc.nb;
    p.tail_pair = sc.nb == 32 && sc.lev_ptr[nlv + 1] - sc.lev_ptr[nlv] == 2;
  }
  const bool lookahead_lists = p.split && nlv >= 2 && (int)sc.tgt_first.size() >= sc.nlev;
  // (dense_dag_items: level 0's tiles and TRSM items, then per level its targets and the next level's)
  if (lookahead_lists) p.n_dag_items = sc.lev_ptr[nlv] + sc.item_ptr[nlv] + sc.tgt_ptr[nlv];
  const bool flow = knobs.want_flow && flow_allowed && lists_fit;
  const bool dag = flow && lookahead_lists && knobs.want_dag && !knobs.force_look2 &&
                   (p.n_dag_items <= kDagMaxItems || knobs.force_dag);
  // k_chol_look's waiting roles take their place from the block index: all of them — first
  // targets, tiles and TRSM items of a level — must be resident at once, whatever the dispatch order
  bool look_fits = lookahead_lists && nlv >= 3;
  for (int l = 0; l + 1 < nlv && look_fits; ++l)
    look_fits = sc.tgt_first[l] + (sc.lev_ptr[l + 2] - sc.lev_ptr[l + 1]) +
                    (sc.item_ptr[l + 2] - sc.item_ptr[l + 1]) <= kFlowResident;
  const bool look = flow && !dag && knobs.want_look2 && look_fits;
  p.fwd = look ? DenseFwd::kLook
        : dag ? DenseFwd::kDag
        : p.split ? DenseFwd::kSplit
        : flow ? DenseFwd::kLevelFlow : DenseFwd::kDiagTrsm;
  p.back = !flow || p.back_t_end == 0 ? DenseBack::kPerLevel
         : sc.max_rows <= kBackGatherMaxRows ? DenseBack::kFlowGather : DenseBack::kFlowOrdered;
  // the cone sweep: measured on the schedule itself, not assumed from its pattern
  if (cone_allowed && lists_fit && p.back_t_end > 0 && sc.max_rows <= kBackGatherMaxRows) {
    const bool short_cones = walk_cones(sc, p.back_t_end, kConeMaxLen, [&](int, const std::vector<int> &cone) {
      ++p.cone_leaves;
      p.cone_max = std::max(p.cone_max, (int)cone.size());
      p.cone_steps += (int)cone.size();
    });
    if (!short_cones) p.cone_leaves = p.cone_max = p.cone_steps = 0;
    p.back_cone = short_cones && p.cone_steps <= kConeMaxWork * p.back_t_end;
  }
  return p;
}

static_assert(4 + kBackGatherMaxRows - 1 <= kConeRec, "a cone record holds every row tile of a gathered column");
static_assert(kConeTailSlots * 32 >= kTailCols, "a slot per tile of the tail block");

void dense_cone_lists(const DenseSchedule &sc, const DenseLaunchPlan &plan, DenseCone &cone) {
  const int t_end = plan.back_t_end, stride = plan.cone_max;
  cone = DenseCone();
  cone.writer.assign((size_t)t_end, -1);
  std::vector<int> step_of((size_t)t_end, -1);  // position -> step in the current cone
  walk_cones(sc, t_end, stride, [&](int leaf, const std::vector<int> &c) {
    const int len = (int)c.size();
    cone.leaf.push_back(c.back());
    cone.len.push_back(len);
    cone.rec.resize((size_t)(leaf + 1) * stride * kConeRec, -1);
    for (int k = 0; k < len; ++k) step_of[c[k]] = k;
    for (int k = 0; k < len; ++k) {
      const int q = c[k];
      int *r = &cone.rec[((size_t)leaf * stride + k) * kConeRec];
      int nrow = 0;
      for (int a = sc.row_ptr[q]; a < sc.row_ptr[q + 1] && sc.rows[a] < sc.ncb; ++a, ++nrow) {
        const int I = sc.rows[a];
        const int slot = I < t_end ? kConeTailSlots + step_of[I] : I - t_end;
        r[4 + nrow] = I | (slot << kConeSlotShift);
      }
      r[0] = q;
      r[1] = nrow;
      r[2] = cone.writer[q] < 0 ? 1 : 0;
      r[3] = len;
      if (cone.writer[q] < 0) cone.writer[q] = leaf;
      const int fill = nrow > 0 ? r[4 + nrow - 1] : (q | ((kConeTailSlots + k) << kConeSlotShift));
      for (int a = nrow; a < kBackGatherMaxRows - 1; ++a) r[4 + a] = fill;
    }
  });
}

DenseLaunchPlan dense_launch_plan_no_tail(const DenseSchedule &sc, DenseKnobs knobs, bool flow_allowed,
                                          const DenseLaunchPlan &uploaded, bool cone_allowed) {
  knobs.want_tail = false;
  return dense_launch_plan(sc, knobs, flow_allowed, /*lists_fit=*/uploaded.tail_levels == 0, cone_allowed);
}

void dense_flow_order(const DenseSchedule &sc, const DenseLaunchPlan &plan, std::vector<int> &order) {
  order.clear();
  for (int l = sc.nlev - plan.tail_levels - 1; l >= 0; --l)
    for (int t = sc.lev_ptr[l]; t < sc.lev_ptr[l + 1]; ++t) order.push_back(t);
}

void dense_dag_items(const DenseSchedule &sc, const DenseLaunchPlan &plan, std::vector<int> &items,
                     std::vector<int> &pre, std::vector<int> &need, std::vector<int> &ntrsm,
                     std::vector<int> &look_need) {
  const int nlv = sc.nlev - plan.tail_levels;
  items.clear();
  pre.assign(std::max<size_t>(1, sc.tgt_J.size()), 0);
  need.assign((size_t)sc.ncb + 1, 0);
  ntrsm.assign((size_t)sc.ncb + 1, 0);
  look_need.assign((size_t)sc.ncb + 1, 0);
  for (size_t q = 0; q < sc.item_t.size(); ++q) ++ntrsm[sc.item_t[q]];
  auto push = [&](int kind, int id) {
    items.push_back(kind);
    items.push_back(id);
  };
  auto tiles_of = [&](int l) {
    for (int t = sc.lev_ptr[l]; t < sc.lev_ptr[l + 1]; ++t) push(0, t);
    for (int q = sc.item_ptr[l]; q < sc.item_ptr[l + 1]; ++q) push(1, q);
  };
  tiles_of(0);
  for (int l = 0; l < nlv; ++l) {
    const int tg0 = sc.tgt_ptr[l], tg1 = sc.tgt_ptr[l + 1], nf = sc.tgt_first[l];
    for (int tg = tg0; tg < tg1; ++tg) pre[tg] = need[sc.tgt_J[tg]];  // (updates of EARLIER levels)
    for (int tg = tg0; tg < tg0 + nf; ++tg) {
      push(2, tg);
      ++look_need[sc.tgt_J[tg]];  // (k_chol_look: the "first" targets of the level before the tile's)
    }
    if (l + 1 < nlv) tiles_of(l + 1);  // the next level's tiles beside the bulk of this level's update
    for (int tg = tg0 + nf; tg < tg1; ++tg) push(2, tg);
    for (int tg = tg0; tg < tg1; ++tg) ++need[sc.tgt_J[tg]];
  }
}

int dense_pick_tile_order(const DenseSchedule &s32, const DenseSchedule &s64, int force_nb) {
  // NARROW patterns (every column tile has at most five row tiles below it besides the rhs
  // block: windows of <= ~15 poses) are latency-bound chains of dependent launches, one set
  // per level, whose cost is a fixed latency plus a term proportional to the tile order: the
  // cheaper chain wins.  Wider and dense patterns are bound by the work per level (row tiles
  // per column, MFMA tile size) and run faster at 64.
  const double level_us[2] = {16.0, 30.0};
  const bool narrow = s32.max_rows <= 6;
  int pick = (narrow && s32.nlev * level_us[0] <= s64.nlev * level_us[1]) ? 0 : 1;
  if (force_nb == 32) pick = 0;
  if (force_nb == 64) pick = 1;
  return pick;
}

}  // namespace ba
