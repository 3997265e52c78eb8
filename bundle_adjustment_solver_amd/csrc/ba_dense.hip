// ba_dense.hip — dense solve of the reduced camera system on gfx950.
//
// Replaces reference core/full_bundle_adjustment_solver.cpp:890-908
// (`x = Am_BCinvBt_mat.ldlt().solve(rhs)`, Eigen's unblocked pivoted LDLT)
// with a blocked right-looking Cholesky whose trailing update runs on the
// fp64 matrix cores (v_mfma_f64_16x16x4_f64).
//
// Storage: column-major lower triangle, `ld` rows, `npad` columns (npad is a
// multiple of 64; padded diagonal = 1).  The right-hand side rides along as
// matrix ROW `npad`, so the forward substitution L z = rhs is performed by the
// panel TRSM / trailing update for free; only L^T x = z needs its own sweep.
// A non-positive pivot (pose without observations -> zero row/column) is
// treated like Eigen's pseudo-inverted D entry: the column and the solution
// component are set to zero.
#include "ba_device.h"
#include "ba_dense_sched.h"
#include "ba_tile16.h"
#include "ba_chol_lds.h"

namespace ba {

namespace {
typedef double v4f64 __attribute__((ext_vector_type(4)));
// Tile order: the kernels exist for 32- and 64-column tiles (ba_dense_tile.inc is
// compiled once per order); ba_finalize picks the order per problem from the
// two level schedules.

// (Re)initialise the tiles of L that the factorisation touches: the
// structurally non-zero tiles of the factor (incl. fill-in), the diagonal tiles
// (unit diagonal on padding columns) and the rhs row block.  Every other tile
// was zeroed once at ba_finalize and is never written.
__global__ __launch_bounds__(256) void k_dense_init(double *L, int ld,
                                                    const int *__restrict__ col_x,
                                                    const int *__restrict__ zt_I,
                                                    const int *__restrict__ zt_J,
                                                    int nb, const int *done) {
  if (done && *done) return;
  const int I = zt_I[blockIdx.x], J = zt_J[blockIdx.x];
  for (int e = threadIdx.x; e < nb * nb; e += 256) {
    const int c = J * nb + e / nb, r = I * nb + e % nb;
    L[(size_t)c * ld + r] = (r == c && col_x[c] < 0) ? 1.0 : 0.0;
  }
}

using tile16::readlane_f64;

#ifdef BA_DENSE_DBG
__device__ long long g_dense_dbg[64];
#define DD_STAMP() { if (threadIdx.x == 0 && blockIdx.x == 0 && t0 == 0 && dd_n < 64) g_dense_dbg[dd_n++] = clock64(); }
#else
#define DD_STAMP()
#endif
namespace nb32 {
constexpr int NB = 32;
#include "ba_dense_tile.inc"
}  // namespace nb32
namespace nb64 {
constexpr int NB = 64;
#include "ba_dense_tile.inc"
}  // namespace nb64
#ifdef BA_DENSE_DBG
extern "C" int ba_debug_read_dense(long long *out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dense_dbg), sizeof(long long) * 64);
}
#endif


// ---- the last levels in ONE workgroup ---------------------------------------
// The level schedule ends with levels of 3, 2, 1 tiles, each of which costs a
// full launch + global round-trip chain (~27 us) for almost no work.  The
// trailing block of the dense image (the tiles of the last levels are its last
// columns: positions are in elimination order) is at that point the Schur
// complement of everything eliminated before, with its right-hand side in the
// rhs row.  This kernel takes the whole block (<= kTailCols columns + the 16-row
// rhs block) into LDS, factors it by left-looking 16-column panels exactly like
// factor_tile_lds (MFMA panel update and TRSM, wave 0 factors the 16x16
// diagonal tiles), forward-substitutes the rhs as one more row tile, and runs
// the block back substitution in the same launch; only x leaves.
// NPt = 16-column panels of the block (compile time: the panel loops unroll and
// their LDS reads pipeline; with run-time bounds the kernel was twice as slow).
template <int NPt, bool PAIR>
__global__ __launch_bounds__(256) void k_chol_tail(const double *L, int ld, int npad, int c0,
                                                   double *xc, double *x,
                                                   const int *__restrict__ col_x, const int *done,
                                                   int *bad) {
  constexpr int nbt = 16 * NPt;
  static_assert(nbt <= kTailCols, "tail block does not fit the LDS image");
  static_assert(!PAIR || NPt >= 4, "a paired first level has two 32-column tiles");
  __shared__ double Lb[kTailCols * kTailLS];             // Lb[c*LS + r], r < nbt: matrix, r >= nbt: rhs block
  __shared__ double Eb[kTailCols / 16][16 * kTailES];    // Eb[p][k*ES + c] = E_pp[k][c], E_pp = L_pp^-T
  __shared__ double xs[kTailCols];
  constexpr int LS = kTailLS, ES = kTailES;
  const int tid = threadIdx.x;
  constexpr int nr = nbt + 16;  // rows of the LDS image; row tile NPt is the rhs block
  // the whole block is requested before anything waits (one load per
  // iteration followed by its LDS store would pay ~40 memory latencies in a row)
  constexpr int kLd = (nbt * nr + 255) / 256;
  double lv[kLd];
#pragma unroll
  for (int k = 0; k < kLd; ++k) {
    const int e = tid + 256 * k;
    const int c = e / nr, rr = e - c * nr;
    const int row = rr < nbt ? c0 + rr : npad + (rr - nbt);
    lv[k] = (e < nbt * nr && rr >= c) ? L[(size_t)(c0 + c) * ld + row] : 0.0;
  }
  if (done && *done) return;
#pragma unroll
  for (int k = 0; k < kLd; ++k) {
    const int e = tid + 256 * k;
    const int c = e / nr, rr = e - c * nr;
    if (e < nbt * nr) Lb[c * LS + rr] = lv[k];
  }
  for (int e = tid; e < (kTailCols / 16) * 16 * ES; e += 256) (&Eb[0][0])[e] = 0.0;
  __syncthreads();
  chol_lds_factor_solve<NPt, PAIR, kTailLS>(Lb, Eb, xs, bad);
  __syncthreads();
  if (tid < nbt) {
    xc[c0 + tid] = xs[tid];
    const int xi = col_x[c0 + tid];
    if (xi >= 0) x[xi] = xs[tid];
  }
}

}  // namespace

void launch_dense_init(double *L, int ld, const int *col_x, const int *zt_I,
                       const int *zt_J, int n_zt, int nb, const int *done_flag,
                       hipStream_t s) {
  if (n_zt > 0)
    BA_LAUNCH(K_DENSE_INIT, k_dense_init, dim3(n_zt), dim3(256), s, L, ld, col_x,
                       zt_I, zt_J, nb, done_flag);
}

namespace {
// NPt is a compile-time parameter of k_chol_tail: 64 columns, 96, or 96 with a paired first level.
auto tail_kernel(const DenseLaunchPlan &pl) {
  if (pl.tail_cols == 64) return k_chol_tail<4, false>;
  return !pl.tail_pair ? k_chol_tail<6, false> : k_chol_tail<6, true>;
}

// The kernels of one tile order (ba_dense_tile.inc, compiled once per order).
struct Nb32 {
  static constexpr int NP = nb32::NP;
  static constexpr auto diag = nb32::k_chol_diag;
  static constexpr auto trsm = nb32::k_chol_trsm;
  static constexpr auto update = nb32::k_chol_update;
  static constexpr auto look = nb32::k_chol_look;
  static constexpr auto dag = nb32::k_chol_dag;
  static constexpr auto level_flow = nb32::k_chol_level_flow;
  static constexpr auto diag_trsm = nb32::k_chol_diag_trsm;
  static constexpr auto back_flow_ordered = nb32::k_chol_back_flow<true>;
  static constexpr auto back_flow_gather = nb32::k_chol_back_flow<false>;
  static constexpr auto back = nb32::k_chol_back;
  static constexpr auto back_cone = nb32::k_chol_back_cone;
};
struct Nb64 {
  static constexpr int NP = nb64::NP;
  static constexpr auto diag = nb64::k_chol_diag;
  static constexpr auto trsm = nb64::k_chol_trsm;
  static constexpr auto update = nb64::k_chol_update;
  static constexpr auto look = nb64::k_chol_look;
  static constexpr auto dag = nb64::k_chol_dag;
  static constexpr auto level_flow = nb64::k_chol_level_flow;
  static constexpr auto diag_trsm = nb64::k_chol_diag_trsm;
  static constexpr auto back_flow_ordered = nb64::k_chol_back_flow<true>;
  static constexpr auto back_flow_gather = nb64::k_chol_back_flow<false>;
  static constexpr auto back = nb64::k_chol_back;
  static constexpr auto back_cone = nb64::k_chol_back_cone;
};

// Level-scheduled, structure-aware blocked Cholesky (see ba_dense_sched.h): the forward
// sweep over the non-tail levels, k_chol_tail, the backward sweep, as `pl` says.
template <class K>
void run_plan(double *L, int npad, int ld, double *Ldiag, double *x, const int *done,
              const DenseSchedule &sc, const DenseDev &dd, const DenseLaunchPlan &pl, hipStream_t s) {
  int *bad = dd.bad_pivots;
  const int row_limit = npad + 16;  // rows that carry data (rhs = row npad)
  const int nlv = sc.nlev - pl.tail_levels;
  const int gen_now = ++dd.flow_gen;  // generation number of this solve (flags are never reset)
  // the role in a dataflow launch: the block index while the grid is resident, else a ticket
  auto ticket = [&](int workgroups, int *counter) {
    return (workgroups <= kFlowResident && !pl.force_ticket) ? nullptr : counter;
  };
  auto diag_and_trsm = [&](int l) {
    const int t0 = sc.lev_ptr[l], nt = sc.lev_ptr[l + 1] - t0;
    const int it0 = sc.item_ptr[l], ni = sc.item_ptr[l + 1] - it0;
    BA_LAUNCH(K_CHOL_DIAG, K::diag, dim3(nt), dim3(256), s, L, ld, t0, Ldiag, done, bad);
    if (ni > 0)
      BA_LAUNCH(K_CHOL_TRSM, K::trsm, dim3(ni), dim3(K::NP * 64), s, L, ld, row_limit, it0, dd.item_t,
                dd.item_I, Ldiag, done);
  };
  auto update = [&](int l) {
    const int tg0 = sc.tgt_ptr[l], ng = sc.tgt_ptr[l + 1] - tg0;
    if (ng > 0)
      BA_LAUNCH(K_CHOL_UPDATE, K::update, dim3(ng), dim3(256), s, L, ld, tg0, dd.tgt_desc, dd.src_t, done);
  };
  switch (pl.fwd) {
    case DenseFwd::kLook:
      diag_and_trsm(0);
      for (int l = 0; l + 1 < nlv; ++l) {
        const int tg0 = sc.tgt_ptr[l], ng = sc.tgt_ptr[l + 1] - tg0, nf = sc.tgt_first[l];
        const int t1 = sc.lev_ptr[l + 1], nt1 = sc.lev_ptr[l + 2] - t1;
        const int it1 = sc.item_ptr[l + 1], ni1 = sc.item_ptr[l + 2] - it1;
        BA_LAUNCH(K_CHOL_UPDATE, K::look, dim3(nt1 + ni1 + ng), dim3(256), s, L, ld, row_limit, nf, t1, nt1,
                  it1, ni1, tg0, dd.item_t, dd.item_I, Ldiag, dd.tgt_desc, dd.src_t, dd.look_need, done, bad,
                  dd.dag_dflags, dd.fwd_cnt, gen_now);
      }
      update(nlv - 1);
      break;
    case DenseFwd::kDag:
      BA_LAUNCH(K_CHOL_UPDATE, K::dag, dim3(pl.n_dag_items), dim3(256), s, L, ld, row_limit,
                (const int2 *)dd.dag_items, pl.n_dag_items, dd.item_t, dd.item_I, dd.dag_ntrsm, Ldiag,
                dd.tgt_desc, dd.src_t, dd.upd_pre, dd.col_need, done, bad, dd.fwd_flags, dd.dag_dflags,
                dd.dag_tcnt, dd.fwd_cnt, dd.fwd_ticket, gen_now);
      break;
    case DenseFwd::kLevelFlow:  // factorisation + TRSM and the updates that consume them
      for (int l = 0; l < nlv; ++l) {
        const int t0 = sc.lev_ptr[l], nt = sc.lev_ptr[l + 1] - t0;
        const int tg0 = sc.tgt_ptr[l], ng = sc.tgt_ptr[l + 1] - tg0;
        BA_LAUNCH(K_CHOL_DIAG_TRSM, K::level_flow, dim3(nt + ng), dim3(256), s, L, ld, npad, t0, nt, tg0, ng,
                  dd.row_desc, dd.rows, Ldiag, dd.tgt_desc, dd.src_t, done, bad, dd.fwd_flags,
                  ticket(nt + ng, dd.fwd_ticket), gen_now);
      }
      break;
    case DenseFwd::kDiagTrsm:
      for (int l = 0; l < nlv; ++l) {
        const int t0 = sc.lev_ptr[l], nt = sc.lev_ptr[l + 1] - t0;
        BA_LAUNCH(K_CHOL_DIAG_TRSM, K::diag_trsm, dim3(nt), dim3(256), s, L, ld, npad, t0, dd.row_desc,
                  dd.rows, Ldiag, done, bad);
        update(l);
      }
      break;
    case DenseFwd::kSplit:
      for (int l = 0; l < nlv; ++l) {
        diag_and_trsm(l);
        update(l);
      }
      break;
  }
  if (pl.tail_levels > 0)
    BA_LAUNCH(K_CHOL_TAIL, tail_kernel(pl), dim3(1), dim3(256), s, L, ld, npad, pl.tail_c0, dd.xc, x, dd.col_x,
              done, bad);
  const int n_back = pl.back_t_end;  // positions of the dataflow launch, top level first in dd.flow_order
  const bool counted = pl.fwd == DenseFwd::kLook || pl.fwd == DenseFwd::kDag;  // (the sweep resets fwd_cnt)
  if (pl.back_cone) {  // (decided with back_t_end > 0: an empty sweep launches nothing)
    BA_LAUNCH(K_CHOL_BACK, K::back_cone, dim3(pl.cone_leaves), dim3(256), s, L, ld, npad, dd.cone_rec, pl.cone_max,
              pl.back_t_end, (sc.ncb - pl.back_t_end) * sc.nb, Ldiag, dd.xc, x, dd.col_x, done,
              counted ? dd.fwd_cnt : nullptr, dd.n_fwd_cnt);
    return;
  }
  switch (pl.back) {
    case DenseBack::kFlowGather:
    case DenseBack::kFlowOrdered:
      BA_LAUNCH(K_CHOL_BACK, pl.back == DenseBack::kFlowOrdered ? K::back_flow_ordered : K::back_flow_gather,
                dim3(n_back), dim3(256), s, L, ld, npad, dd.flow_order, n_back, pl.back_t_end, dd.back_desc,
                dd.rows, Ldiag, dd.xc, x, dd.col_x, done, dd.flow_flags, ticket(n_back, dd.flow_ticket), gen_now,
                bad, counted ? dd.fwd_cnt : nullptr, dd.n_fwd_cnt);
      break;
    case DenseBack::kPerLevel:
      for (int l = nlv - 1; l >= 0; --l) {
        const int t0 = sc.lev_ptr[l], nt = sc.lev_ptr[l + 1] - t0;
        BA_LAUNCH(K_CHOL_BACK, K::back, dim3(nt), dim3(256), s, L, ld, npad, t0, dd.back_desc, dd.rows, Ldiag,
                  dd.xc, x, dd.col_x, done);
      }
      break;
  }
}
}  // namespace

void dense_factor_solve(double *L, int npad, int ld, double *Ldiag, double *x, const int *done,
                        const DenseSchedule &sc, const DenseDev &dd, const DenseLaunchPlan &plan,
                        hipStream_t s) {
  if (sc.nb == 32)
    run_plan<Nb32>(L, npad, ld, Ldiag, x, done, sc, dd, plan, s);
  else
    run_plan<Nb64>(L, npad, ld, Ldiag, x, done, sc, dd, plan, s);
}

void launch_dense_solve(const DevProblem &d, const DenseSchedule &sc,
                        const DenseDev &dd, hipStream_t s) {
  dense_factor_solve(d.L, d.npad, d.ld, d.Ldiag, d.x, &d.ctrl->done, sc, dd, dd.plan[dd.flow_ok], s);
}

}  // namespace ba
