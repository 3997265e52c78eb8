// ba_dense_sched.h — host-side symbolic analysis for the structure-aware,
// level-scheduled Cholesky of the reduced camera system (ba_dense.hip).
//
// The reference solves the reduced camera system with a dense, sequential,
// unblocked LDLT (reference core/full_bundle_adjustment_solver.cpp:905).  The
// matrix is block sparse: two poses couple only through landmarks they both
// observe.  Here the 6x6 pose blocks are grouped into 64-column TILES
// (kPosesPerTile poses + padding); on the tile graph we compute
//   1. a parallel minimum-degree ordering: each LEVEL is an independent set of
//      low-degree tiles (for a band matrix this is odd-even cyclic reduction,
//      log2(n) levels; for a dense matrix it degenerates to one tile per level,
//      i.e. the classic right-looking sweep);
//   2. the symbolic factor (fill-in) under that ordering;
//   3. static work lists per level: diagonal tiles, TRSM items, and update
//      TARGETS with their source panels (target-centric so that tiles shared by
//      several panels of one level are summed by one workgroup in fixed order:
//      deterministic, no atomics).
// Skipping structurally zero tiles is exact (they are zero in a dense
// factorisation too); only the floating-point summation order differs from the
// natural ordering.
#ifndef BA_DENSE_SCHED_H_
#define BA_DENSE_SCHED_H_

#include <cstdint>
#include <vector>

namespace ba {

// Tile order nb = 32 (5 poses + 2 padding columns) or 64 (10 poses + 4): chosen
// per problem by ba_finalize from the two level schedules.
inline int dense_poses_per_tile(int nb) { return nb == 32 ? 5 : 10; }
inline int dense_ws_per_block(int nb) { return nb * nb + (nb / 16) * 256; }

struct DenseSchedule {
  int nb = 32;    // tile order the schedule was built for
  int ncb = 0;    // tiles (the rhs row block has index ncb)
  int nlev = 0;
  std::vector<int> pos_of_tile;  // original tile/group -> elimination position
  std::vector<int> tile_at_pos;  // inverse
  std::vector<int> lev_ptr;      // nlev+1: positions [lev_ptr[l], lev_ptr[l+1])
  std::vector<int> row_ptr, rows;  // per position: non-zero row tiles below
                                   // (ascending positions), rhs block last
  std::vector<int> item_ptr, item_t, item_I;        // TRSM items per level
  std::vector<int> tgt_ptr, tgt_I, tgt_J;           // update targets per level
  std::vector<int> tgt_first;                       // per level: its first targets that lie in a column of the NEXT level
  std::vector<int> tgt_src_ptr, src_t;              // sources of each target
  // The same lists as fixed 8-int records, so that a workgroup reaches its data
  // after ONE dependent load:
  //   tgt_desc[8 tg ..] = { I, J, nsrc, src_begin, first four sources (-1 pad) }
  //   back_desc[8 p ..] = { nrow (without the rhs block), row_begin, first six rows }
  std::vector<int> tgt_desc, back_desc;
  //   row_desc[16 p ..] = { nrow (incl. the rhs block), row_begin, 0.., first eight row tiles at [8..15] }
  std::vector<int> row_desc;
  int max_rows = 0;  // most row tiles (incl. the rhs block) below any tile
  double fill = 1.0;        // non-zero factor tiles / all lower tiles
  double flops = 0.0;       // executed flops of factor + solves (estimate)
};

// `adj` is the symmetric ncb x ncb tile adjacency (non-zero off-diagonal
// tiles), row-major bytes.  `natural_order` = keep the given order and put
// every tile in its own level (debug / dense comparison).  `order` = 's': the strict
// ordering, 'r': the relaxed one, 0: whichever gives the shorter chain of launches
// (DenseKnobs::natural, DenseKnobs::order).
void build_dense_schedule(int ncb, const std::vector<uint8_t> &adj,
                          bool natural_order, int nb, DenseSchedule &s, char order = 0);

// ---- which kernels run a schedule (launched by dense_factor_solve, ba_dense.hip) ----
// DESIGN.md ("launch paths of the dense solve") has the measurements behind the defaults.

// Columns of the block that k_chol_tail factors in LDS (ba_chol_lds.h).
constexpr int kTailCols = 96;
// Workgroups of a dataflow launch that are certainly resident at once on the part (256
// CUs x 2 workgroups of 256 threads at the kernels' register budgets, with a margin):
// up to here the role is the block index, beyond it a ticket (ba_dense_tile.inc).
constexpr int kFlowResident = 448;
// k_chol_dag takes the forward sweep up to this many items, k_chol_look beyond.
constexpr int kDagMaxItems = 16384;
// The backward dataflow sweep gathers up to this many row tiles per column (incl. the rhs
// block) and consumes them in order beyond.
constexpr int kBackGatherMaxRows = 12;
// Row tiles per column (incl. the rhs block) that a tile's own workgroup solves: they must
// fit its prefetched passes, 4 passes x (4 waves / (nb / 16)) tiles.
inline int dense_fused_max_rows(int nb) { return 4 * (4 / (nb / 16)); }
// The cone sweep (k_chol_back_cone: one workgroup per leaf solves its own chain of ancestors,
// no hand-off between workgroups) is taken while the longest cone has at most kConeMaxLen
// steps and the steps of all cones together are at most kConeMaxWork times the non-tail tiles
// (launch-path table, has the numbers behind both).
constexpr int kConeMaxLen = 8;
constexpr double kConeMaxWork = 4.0;
// One step of a cone is a record of kConeRec ints (see DenseCone); a row tile is packed as
// position | slot << kConeSlotShift.
constexpr int kConeRec = 16;
constexpr int kConeSlotShift = 20;
// Slots of x in front of a cone's own steps: the tiles of the tail block (kTailCols / 32).
constexpr int kConeTailSlots = 3;

// The BA_DENSE_* environment variables (part of Knobs, ba_knobs.h: read once per handle).
struct DenseKnobs {
  bool want_split = false;                      // SPLIT=1: separate diagonal and TRSM launches
  bool want_tail = true;                        // TAIL=0: no k_chol_tail
  bool want_flow = true;                        // FLOW=0: no dataflow launch
  bool want_dag = true, force_dag = false;      // DAG=0: no k_chol_dag; =1: also beyond kDagMaxItems
  bool want_look2 = true, force_look2 = false;  // LOOK2=0: no k_chol_look; =1: instead of k_chol_dag too
  bool force_ticket = false;                    // TICKET=1: tickets even when the grid is resident (test knob)
  bool natural = false, full = false;           // NATURAL=1, FULL=1: debug orderings / patterns
  int nb = 0;                                   // NB=32|64: tile order (0: dense_pick_tile_order decides)
  char order = 0;                               // ORDER=strict|relaxed: 's' / 'r' (developer knob)
  static DenseKnobs from_env();
};

// BA_DENSE_CONE=0 forbids the cone sweep (k_chol_back_cone).  A record of its own beside
// DenseKnobs (Knobs::cone, ba_knobs.h: read once per handle), handed to dense_launch_plan
// as `cone_allowed`.
struct ConeKnobs {
  bool want = true;
  static ConeKnobs from_env();
};

enum class DenseFwd {
  kLook,       // k_chol_look: one launch per level with lookahead into the next
  kDag,        // k_chol_dag: every non-tail level in one dataflow launch
  kLevelFlow,  // k_chol_level_flow: one dataflow launch per level
  kDiagTrsm,   // k_chol_diag_trsm + k_chol_update per level
  kSplit       // k_chol_diag + k_chol_trsm + k_chol_update per level
};
enum class DenseBack {
  kFlowGather,   // k_chol_back_flow<false>: one launch, waits for all row tiles, then gathers
  kFlowOrdered,  // k_chol_back_flow<true>: one launch, consumes the row tiles as their flags come up
  kPerLevel      // k_chol_back per level
};
const char *dense_fwd_name(DenseFwd f);
const char *dense_back_name(DenseBack b);

struct DenseLaunchPlan {
  bool split = false;  // the tile's workgroup does not solve its own row tiles
  // the last levels (at least two, together 64 or 96 columns) go to k_chol_tail
  int tail_levels = 0, tail_cols = 0, tail_c0 = 0;
  bool tail_pair = false;  // two (independent) 32-column tiles in the block's first level: panels side by side
  int back_t_end = 0;      // the sweeps cover the positions [0, back_t_end): the non-tail levels
  int n_dag_items = 0;     // items of dense_dag_items for this tail; 0: k_chol_dag / k_chol_look do not apply
  DenseFwd fwd = DenseFwd::kSplit;
  DenseBack back = DenseBack::kPerLevel;
  bool force_ticket = false;
  // The backward sweep is ONE k_chol_back_cone launch of cone_leaves workgroups instead of
  // `back` (which keeps its value: the form taken when the cone sweep is forbidden).  It has no
  // generation number and no flags, so it does not depend on `flow_allowed`.
  bool back_cone = false;
  int cone_leaves = 0, cone_max = 0, cone_steps = 0;  // leaves, steps of the longest cone, of all cones
};

// The one place that decides.  `flow_allowed`: false while a captured graph is in use (the
// generation number of a dataflow launch is a kernel argument).  `lists_fit`: the uploaded
// dataflow lists (dense_flow_order, dense_dag_items) and cone lists (dense_cone_lists) were
// built for this plan's tail; a plan whose tail differs from the uploaded one takes no
// dataflow launch and no cone sweep.
// `cone_allowed`: ConeKnobs::want.
DenseLaunchPlan dense_launch_plan(const DenseSchedule &sc, const DenseKnobs &knobs, bool flow_allowed,
                                  bool lists_fit = true, bool cone_allowed = true);
// The plan that hands no level to k_chol_tail (which keeps its block's factor in LDS: only
// x leaves), for a caller that needs the whole factor in the image.  `uploaded`: the plan
// the device lists were built for.
DenseLaunchPlan dense_launch_plan_no_tail(const DenseSchedule &sc, DenseKnobs knobs, bool flow_allowed,
                                          const DenseLaunchPlan &uploaded, bool cone_allowed = true);

// Positions of the backward sweep's dataflow launch, top level first (plan.back_t_end of them).
void dense_flow_order(const DenseSchedule &sc, const DenseLaunchPlan &plan, std::vector<int> &order);
// Lists of the cone sweep (k_chol_back_cone).  A LEAF is a non-tail position that is no row
// tile of another non-tail position; its CONE is the closure of rows[] over the non-tail
// positions, in descending position, the leaf itself last: every row tile of a step is an
// earlier step of the same cone or a tile of the tail block.  A workgroup keeps x in slots of
// LDS: slot I - back_t_end for a tail tile I (read from xc), slot kConeTailSlots + k for step k.
//   rec[kConeRec * (leaf * plan.cone_max + k) ..] = { position, nrow (without the rhs block),
//       1 if this leaf stores the position's x, steps of the cone,
//       row tiles as position | slot << kConeSlotShift (entries beyond nrow repeat the last
//       one; with no row tile: the step itself), -1 pad }
// — a fixed stride per leaf, so that a workgroup reaches a step after ONE load that depends
// on nothing but its block index.  Exactly one leaf, the lowest whose cone holds it, stores a
// position: writer[position] = index of that leaf.  Call only if plan.back_cone.
struct DenseCone {
  std::vector<int> leaf;    // positions of the leaves, ascending
  std::vector<int> len;     // steps per leaf
  std::vector<int> rec;
  std::vector<int> writer;  // per non-tail position
};
void dense_cone_lists(const DenseSchedule &sc, const DenseLaunchPlan &plan, DenseCone &cone);
// Work list of the three-kernel path as one dataflow launch (k_chol_dag): items = {kind, index}
// pairs in lookahead order (kind 0: tile position, 1: TRSM item, 2: update target), pre[tg] =
// updates of earlier levels on the target's column, need[p] = all updates on position p's column,
// ntrsm[p] = TRSM items of position p, look_need[p] = the previous level's first targets in
// p's column (k_chol_look).  Call only if plan.n_dag_items > 0.
void dense_dag_items(const DenseSchedule &sc, const DenseLaunchPlan &plan, std::vector<int> &items,
                     std::vector<int> &pre, std::vector<int> &need, std::vector<int> &ntrsm,
                     std::vector<int> &look_need);

// Tile order of a problem from its two candidate schedules: 0 (nb32) or 1 (nb64); force_nb
// = 32 | 64 overrides (DenseKnobs::nb).
int dense_pick_tile_order(const DenseSchedule &s32, const DenseSchedule &s64, int force_nb);

}  // namespace ba
#endif
