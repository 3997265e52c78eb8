// ba_api.hip — implementation of the C ABI declared in include/ba_hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ba_device_fn.h"
#include "ba_handle.h"
#include "ba_rel_host.h"

namespace {
thread_local std::string g_err;
}  // namespace
void ba::set_last_error(const std::string &m) { g_err = m; }
int ba::fail(const std::string &m) {
  g_err = m;
  return -1;
}
using ba::fail;
using ba::Mem;

namespace {

int use_device(ba_handle *h) {
  HIP_TRY(hipSetDevice(h->device));
  return 0;
}

// one stage boundary: optional event record
inline void mark(ba_handle *h, int k) {
  if (h->timing) (void)hipEventRecord(h->ev[k], h->stream);
}

int xchg(ba_handle *h, int which) {
  if (!h->ar_fn) return 0;
  void *ptr = which == 0 ? (void *)h->d.Spk : (void *)h->d.scal;
  int rc = h->ar_fn(h->ar_user, which, ptr, h->xbuf_n[which], (void *)h->stream);
  if (rc != 0) return fail("all-reduce hook returned an error");
  return 0;
}

// The main stream waits for the side stream's outstanding work (if any).
void join_side(ba_handle *h) {
  h->tiles_ready = false;  // (every entry point but the LM iteration itself may dirty the factor tiles)
  if (!h->side_pending) return;
  (void)hipStreamWaitEvent(h->stream, h->ev_join, 0);
  h->side_pending = false;
}

// Linearisation at the `sel` parameters on the main stream (blocks of buffer
// lcur ^ sel, cost partials as a by-product).
void enqueue_linearize(ba_handle *h, int sel) {
  const ba::DevProblem &d = h->d;
  ba::launch_lin_landmarks(d, sel, h->stream);  // (k_lin_grp's pose-side rows precede k_pose_finalize)
  ba::launch_lin_poses(d, sel, h->stream);
  if (d.n_obs_lm < d.n_obs) ba::launch_cost(d, sel ? 2 : 0, d.n_obs_lm, h->stream);
}

// Enqueue one LM iteration (reference :709-1007) without host sync.
// On entry the block buffer ctrl->lcur holds the linearisation at the accepted
// parameters (made by ba_lm_begin or, as the trial-point linearisation, by the
// previous iteration).  The iteration damps and inverts with the current lambda,
// forms and solves the reduced system, back-substitutes, writes the trial
// parameters, LINEARISES AT THE TRIAL POINT into the other block buffer — the
// trial cost (reference :927) is the sum of the residual norms that pass computes
// anyway — and takes the trust-region decision, which flips parameter and block
// buffers together on acceptance.  Per iteration one pass over the observations
// less than "cost at the trial point, then linearise again" (reference
// :709-927), and a rejected step costs no second linearisation of the same point.
int enqueue_iteration(ba_handle *h) {
  const ba::DevProblem &d = h->d;
  hipStream_t s = h->stream;
  ba::g_ktimer = h->timing ? &h->kt : nullptr;
  // per-kernel / per-stage timing needs the serial order on one stream; a captured
  // graph cannot wait for an event of the previous replay
  // relative-pose factors (ba_set_relative): their launches sit between the others in
  // stream order, so a handle with factors keeps everything on the main stream
  const bool rel = h->rel.F > 0;
  const bool ov = h->overlap && !h->timing && !h->use_graph && !rel;
  const bool direct = !h->ar_fn;  // single GPU: S, rhs are placed in the dense matrix at once
  h->ddev.flow_ok = !h->use_graph;  // (the dataflow sweep's generation number is a kernel argument)
  mark(h, 0);
  ba::launch_damp_invert(d, s);
  const bool had_side = h->side_pending;
  if (!had_side && !h->tiles_ready)
    ba::launch_dense_init(d.L, d.ld, d.col_x, d.zt_I, d.zt_J, d.n_zt, d.nb, &d.ctrl->done, s);
  h->tiles_ready = false;
  // NO SIDE STREAM when nothing is left for it: single GPU, every landmark with a free
  // pose in a covisibility group (no pose-major pass), no cost pass — the reset of the
  // factor tiles rides in the back-substitution launch (the solve is over by then),
  // the pose-side sums in the k_scalars launch: no fork / join gaps (6 + 8 us at C4).
  const bool no_side = !rel && !h->knobs.run.force_side && !h->ar_fn && d.lin_chunk0 > 0 && d.n_achunk == 0 && d.n_obs_lm == d.n_obs;
  ba::launch_schur_accumulate(d, s);
  join_side(h);  // A_j, a_j of this point and the reset factor tiles come from the side stream
  ba::launch_schur_final(d, direct, s);
  if (rel) ba::launch_rel_offdiag(d, h->rel, direct, s);  // S_jk += -Omega Ad of the accepted point, undamped
  mark(h, 1);
  if (xchg(h, 0)) return -1;
  mark(h, 2);
  if (!direct) ba::launch_scatter(d, s);
  ba::launch_dense_solve(d, h->sched, h->ddev, s);
  mark(h, 3);
  ba::launch_backsub_update(d, s, no_side);  // trial parameters, model terms, step norms
  // the factors' cross term of the model, their linearisation at the trial poses, their norms there
  if (rel) ba::launch_rel_lin(d, h->rel, 1, 3, s);
  mark(h, 4);
  if (no_side) {
    h->tiles_ready = true;
    ba::launch_lin_landmarks(d, 1, s);
  } else if (ov) {
    // pose side of the trial-point linearisation and the reset of the factor
    // tiles: first needed by the NEXT iteration's k_schur_final.  They start after
    // k_lin_landmarks, beside the control step, the damping kernel and the first
    // part of k_schur_lds.
    // (with covisibility groups linearised by k_lin_grp the pose-side sums of the
    //  side stream's k_pose_finalize read that kernel's rows)
    ba::launch_lin_landmarks(d, 1, s);
    if (d.n_obs_lm < d.n_obs) ba::launch_cost(d, 2, d.n_obs_lm, s);
    (void)hipEventRecord(h->ev_fork, s);
    (void)hipStreamWaitEvent(h->side_stream, h->ev_fork, 0);
    ba::launch_dense_init(d.L, d.ld, d.col_x, d.zt_I, d.zt_J, d.n_zt, d.nb, &d.ctrl->done, h->side_stream);
    ba::launch_lin_poses(d, 1, h->side_stream);
    (void)hipEventRecord(h->ev_join, h->side_stream);
    h->side_pending = true;
  } else {
    enqueue_linearize(h, 1);
  }
  mark(h, 5);
  if (h->ar_fn || rel) {
    ba::launch_scalars(d, 1, s);
    mark(h, 6);
    if (xchg(h, 1)) return -1;
    // A_j, a_j of the trial point gain the factors' blocks (k_pose_finalize has run), the
    // scalars their norms and cross term: the decision comes after
    if (rel) ba::launch_rel_gather(d, h->rel, 1, 7, s);
    mark(h, 7);
    ba::launch_control(d, s);
  } else {  // nothing to exchange: the reduction workgroup also takes the LM decision
    ba::launch_scalars_and_control(d, 1, s, no_side ? 1 : -1);
    mark(h, 6);
    mark(h, 7);
  }
  mark(h, 8);
  ba::g_ktimer = nullptr;
  if (h->timing) {
    HIP_TRY(hipStreamSynchronize(s));
    h->kt.collect();
    static const int stage_of[8] = {ST_SCHUR, ST_XCHG, ST_SOLVE, ST_BACKSUB,
                                    ST_BUILD, ST_CTRL, ST_XCHG, ST_CTRL};
    for (int k = 0; k < 8; ++k) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]) == hipSuccess)
        h->stage_ms[stage_of[k]] += ms;
    }
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int push_ctrl(ba_handle *h) {
  HIP_TRY(hipMemcpyAsync(h->d.ctrl, &h->hc, sizeof(ba::DevCtrl),
                         hipMemcpyHostToDevice, h->stream));
  return 0;
}
int pull_ctrl(ba_handle *h) {
  HIP_TRY(hipMemcpyAsync(&h->hc, h->d.ctrl, sizeof(ba::DevCtrl),
                         hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

template <class T>
int download(std::vector<T> &out, const T *dev, size_t n, hipStream_t s) {
  out.resize(n);
  if (n == 0) return 0;
  HIP_TRY(hipMemcpyAsync(out.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

// Device set-up of a dense schedule: the work lists of `dd`, its column -> x map col_x
// (npad entries), the solution in column order xc, the dropped-pivot counter, the order,
// flags and tickets of the dataflow sweeps, the k_chol_dag / k_chol_look items and
// counters and the step records of the cone sweep; fixes the launch plans from the handle's dense knobs.  Everything is allocated on
// the handle (h->upload / h->dalloc, in h->allocs).  Also used by ba_pgraph.hip.
}  // namespace
int ba::upload_dense_schedule(ba_handle *h, const ba::DenseSchedule &sc, const std::vector<int> &col_x,
                              ba::DenseDev &dd) {
  const size_t npad = col_x.size(), ncb = (size_t)std::max(1, sc.ncb);
  constexpr Mem R = Mem::Resident;  // a dense system is pose-sized and shared by every chunk
  if (h->upload(R, &dd.row_ptr, sc.row_ptr) || h->upload(R, &dd.rows, sc.rows) ||
      h->upload(R, &dd.item_t, sc.item_t) || h->upload(R, &dd.item_I, sc.item_I) ||
      h->upload(R, &dd.tgt_I, sc.tgt_I) || h->upload(R, &dd.tgt_J, sc.tgt_J) ||
      h->upload(R, &dd.tgt_src_ptr, sc.tgt_src_ptr) || h->upload(R, &dd.src_t, sc.src_t) ||
      h->upload(R, &dd.tgt_desc, sc.tgt_desc) || h->upload(R, &dd.back_desc, sc.back_desc) ||
      h->upload(R, &dd.row_desc, sc.row_desc) || h->upload(R, &dd.col_x, col_x) ||
      h->dalloc(R, &dd.xc, npad) || h->dalloc(R, &dd.bad_pivots, (size_t)1))
    return -1;
  HIP_TRY(hipMemset(dd.xc, 0, npad * sizeof(double)));
  HIP_TRY(hipMemset(dd.bad_pivots, 0, sizeof(int)));
  for (int flow_ok = 0; flow_ok < 2; ++flow_ok) dd.plan[flow_ok] = ba::dense_launch_plan(sc, h->knobs.dense, flow_ok != 0, /*lists_fit=*/true, h->knobs.cone.want);
  const ba::DenseLaunchPlan &plan = dd.plan[1];  // (plan[0] has the same tail, lists and cone sweep: its other launches are per level)
  std::vector<int> order;
  ba::dense_flow_order(sc, plan, order);
  dd.flow_gen = 0;
  if (h->upload(R, &dd.flow_order, order) || h->dalloc(R, &dd.flow_flags, ncb) || h->dalloc(R, &dd.flow_ticket, (size_t)1) ||
      h->dalloc(R, &dd.fwd_flags, ncb) || h->dalloc(R, &dd.fwd_ticket, (size_t)1))
    return -1;
  HIP_TRY(hipMemset(dd.flow_flags, 0, ncb * sizeof(int)));
  HIP_TRY(hipMemset(dd.flow_ticket, 0, sizeof(int)));
  HIP_TRY(hipMemset(dd.fwd_flags, 0, ncb * sizeof(int)));
  HIP_TRY(hipMemset(dd.fwd_ticket, 0, sizeof(int)));
  if (plan.n_dag_items > 0) {
    std::vector<int> items, pre, need, ntrsm, lneed;
    ba::dense_dag_items(sc, plan, items, pre, need, ntrsm, lneed);
    dd.n_fwd_cnt = (int)need.size();
    if (h->upload(R, &dd.dag_items, items) || h->upload(R, &dd.upd_pre, pre) || h->upload(R, &dd.col_need, need) ||
        h->upload(R, &dd.dag_ntrsm, ntrsm) || h->upload(R, &dd.look_need, lneed) || h->dalloc(R, &dd.fwd_cnt, need.size()) ||
        h->dalloc(R, &dd.dag_dflags, need.size()) || h->dalloc(R, &dd.dag_tcnt, need.size()))
      return -1;
    HIP_TRY(hipMemset(dd.fwd_cnt, 0, need.size() * sizeof(int)));
    HIP_TRY(hipMemset(dd.dag_dflags, 0, need.size() * sizeof(int)));
    HIP_TRY(hipMemset(dd.dag_tcnt, 0, need.size() * sizeof(int)));
  }
  if (plan.back_cone) {
    ba::DenseCone cone;
    ba::dense_cone_lists(sc, plan, cone);
    if (h->upload(R, &dd.cone_rec, cone.rec)) return -1;
  }
  return 0;
}
namespace {
using ba::upload_dense_schedule;

// ---- the steps of ba_finalize, in the order it runs them.  Every dalloc / upload names
// its residency (ba_handle.h: Mem); the ORDER of the chunk allocations fixes the layout
// of a streamed chunk's host image (ba_stream.hip).

// The plan of this handle's shard, and the sizes the device code reads from it.
int finalize_plan(ba_handle *h) {
  ba::PlanInput in;
  in.n_cam = h->n_cam;
  in.n_pose = h->n_pose;
  in.pose_fixed = h->pose_fixed.data();
  in.n_pt = h->n_pt;
  in.pt_fixed = h->pt_fixed.data();
  in.n_obs = h->n_obs;
  in.obs_cam = h->obs_cam.data();
  in.obs_pose = h->obs_pose.data();
  in.obs_pt = h->obs_pt.data();
  in.obs_uv = h->obs_uv.data();
  in.rank = h->rank;
  in.world = h->world;
  in.n_rel = (int64_t)h->rel_j.size();
  in.rel_j = h->rel_j.data();
  in.rel_k = h->rel_k.data();
  std::string err = ba::build_plan(in, h->knobs.plan, h->plan);
  if (!err.empty()) return fail("ba_finalize: " + err);
  const ba::Plan &pl = h->plan;
  ba::DevProblem &d = h->d;
  std::memset(&d, 0, sizeof(d));
  d.n_cam = pl.n_cam; d.n_pose = pl.n_pose; d.N = pl.N; d.n_pt = pl.n_pt;
  d.M = pl.M; d.M_global = pl.M_global; d.n_obs = pl.n_obs;
  d.n_obs_opt = pl.n_obs_opt; d.n_obs_global = pl.n_obs_global; d.P = pl.P;
  d.n_pobs = pl.n_pobs; d.T = pl.T; d.B = pl.B;
  d.n_achunk = (int)pl.achunk_pose.size();
  d.n_tchunk = (int)pl.tchunk_blk.size();
  return 0;
}

// Cameras, poses and points in the internal order (both parameter buffers).
int upload_parameters(ba_handle *h) {
  const ba::Plan &pl = h->plan;
  ba::DevProblem &d = h->d;
  std::vector<double> cams((size_t)pl.n_cam * 16);
  for (int c = 0; c < pl.n_cam; ++c) {
    std::memcpy(&cams[(size_t)c * 16], &h->cam_intr[(size_t)c * 4], 4 * sizeof(double));
    std::memcpy(&cams[(size_t)c * 16 + 4], &h->cam_T[(size_t)c * 12], 12 * sizeof(double));
  }
  if (h->upload(Mem::Resident, &d.cams, cams)) return -1;
  std::vector<double> poses((size_t)pl.n_pose * 12);
  for (int p = 0; p < pl.n_pose; ++p)
    std::memcpy(&poses[(size_t)p * 12], &h->pose_T[(size_t)pl.pose_user_of_int[p] * 12],
                12 * sizeof(double));
  if (h->upload(Mem::Resident, &d.poses[0], poses) || h->upload(Mem::Resident, &d.poses[1], poses)) return -1;
  std::vector<double> pts((size_t)pl.n_pt * 3);
  for (int q = 0; q < pl.n_pt; ++q)
    std::memcpy(&pts[(size_t)q * 3], &h->pt_X[(size_t)pl.pt_user_of_int[q] * 3],
                3 * sizeof(double));
  if (h->upload(Mem::ChunkState, &d.pts[0], pts) || h->upload(Mem::ChunkState, &d.pts[1], pts)) return -1;
  return 0;
}

// 16-int record per S block: its pose pair, its slot contributions (the first 8 inline)
// and its triangle chunks
std::vector<int32_t> make_blk_desc(const ba::Plan &pl) {
  std::vector<int32_t> bd((size_t)pl.B * 16, 0);
  for (int64_t bk = 0; bk < pl.B; ++bk) {
    int32_t *r = bd.data() + 16 * bk;
    const int64_t c0 = pl.blk_contrib_ptr[bk], c1 = pl.blk_contrib_ptr[bk + 1];
    r[0] = pl.sblk_j[bk];
    r[1] = pl.sblk_k[bk];
    r[2] = (int32_t)c0;
    r[3] = (int32_t)(c1 - c0);
    r[4] = pl.sblk_tchunk_ptr[bk];
    r[5] = pl.sblk_tchunk_ptr[bk + 1] - pl.sblk_tchunk_ptr[bk];
    for (int t = 0; t < 8; ++t) r[8 + t] = c0 + t < c1 ? pl.contrib_slot[c0 + t] : 0;
  }
  return bd;
}

// first pair / observation / landmark and the counts of every landmark chunk
std::vector<ba::DevProblem::LmChunk> make_lm_chunks(const ba::Plan &pl) {
  std::vector<ba::DevProblem::LmChunk> lc(pl.bchunk_lm.size() - 1);
  for (size_t c = 0; c < lc.size(); ++c) {
    const int l0 = pl.bchunk_lm[c], l1 = pl.bchunk_lm[c + 1];
    lc[c].pb = pl.lm_pair_ptr[l0];
    lc[c].ob = pl.lm_obs_ptr[l0];
    lc[c].l0 = l0;
    lc[c].nl = l1 - l0;
    lc[c].np = (int32_t)(pl.lm_pair_ptr[l1] - pl.lm_pair_ptr[l0]);
    lc[c].no = (int32_t)(pl.lm_obs_ptr[l1] - pl.lm_obs_ptr[l0]);
  }
  return lc;
}

// Structure, first half: observations and the index lists over them.  Where the planner's
// element type differs from the device's (flat int32 / double vectors, its own mirror of a
// descriptor) the static_asserts pin the layout and the upload takes the host pointer and
// the record count.
int upload_observation_lists(ba_handle *h) {
  const ba::Plan &pl = h->plan;
  ba::DevProblem &d = h->d;
  static_assert(sizeof(int4) == 16 && sizeof(double2) == 16 && sizeof(int2) == 8, "layout");
  if (h->upload(Mem::ChunkConst, &d.obs_idx, pl.obs_idx.data(), (size_t)pl.n_obs) ||
      h->upload(Mem::ChunkConst, &d.obs_uv, pl.obs_uv.data(), (size_t)pl.n_obs))
    return -1;
  // slim landmark-major record for the cost kernel (no pair id, 8 bytes)
  if (!pl.obs_cp.empty() && pl.n_obs > 0 && !h->knobs.run.cost_wide)  // (filled by the planner's threaded pass)
    if (h->upload(Mem::ChunkConst, &d.obs_cp, pl.obs_cp.data(), (size_t)pl.n_obs)) return -1;
  if (h->upload(Mem::ChunkConst, &d.pobs_idx, pl.pobs_idx.data(), (size_t)pl.n_pobs) ||
      h->upload(Mem::ChunkConst, &d.pobs_uv, pl.pobs_uv.data(), (size_t)pl.n_pobs) ||
      h->upload(Mem::ChunkConst, &d.lm_obs_ptr, pl.lm_obs_ptr) ||
      h->upload(Mem::ChunkConst, &d.lm_pair_ptr, pl.lm_pair_ptr) ||
      h->upload(Mem::ChunkConst, &d.pair_pose, pl.pair_pose) || h->upload(Mem::ChunkConst, &d.pair_lm, pl.pair_lm) ||
      h->upload(Mem::ChunkConst, &d.achunk_pose, pl.achunk_pose) ||
      h->upload(Mem::ChunkConst, &d.achunk_begin, pl.achunk_begin) ||
      h->upload(Mem::ChunkConst, &d.achunk_end, pl.achunk_end) ||
      h->upload(Mem::ChunkConst, &d.pose_achunk_ptr, pl.pose_achunk_ptr))
    return -1;
  // the block numbering of S is global and k_scatter reads it while no particular chunk
  // is resident: DESIGN.md §6b "Residency"
  if (h->upload(Mem::Resident, &d.sblk_j, pl.sblk_j) || h->upload(Mem::Resident, &d.diag_blk, pl.diag_blk) ||
      h->upload(Mem::Resident, &d.sblk_k, pl.sblk_k))
    return -1;
  if (pl.contrib_slot.size() >= (size_t)INT32_MAX) return fail("too many slot contributions for int32 indices");
  if (h->upload(Mem::ChunkConst, &d.tri_p, pl.tri_p) || h->upload(Mem::ChunkConst, &d.tri_q, pl.tri_q) ||
      h->upload(Mem::ChunkConst, &d.tchunk_blk, pl.tchunk_blk) ||
      h->upload(Mem::ChunkConst, &d.tchunk_begin, pl.tchunk_begin) ||
      h->upload(Mem::ChunkConst, &d.tchunk_end, pl.tchunk_end) ||
      h->upload(Mem::ChunkConst, &d.sblk_tchunk_ptr, pl.sblk_tchunk_ptr) ||
      h->upload(Mem::ChunkConst, &d.ltri, pl.ltri) || h->upload(Mem::ChunkConst, &d.chunk_sp, pl.chunk_sp) ||
      h->upload(Mem::ChunkConst, &d.sup_lane, pl.sup_lane) ||
      h->upload(Mem::ChunkConst, &d.blk_contrib_ptr, pl.blk_contrib_ptr) ||
      h->upload(Mem::ChunkConst, &d.contrib_slot, pl.contrib_slot) ||
      h->upload(Mem::ChunkConst, &d.blk_desc, make_blk_desc(pl)) ||
      h->upload(Mem::ChunkConst, &d.bchunk_lm, pl.bchunk_lm) ||
      h->upload(Mem::ChunkConst, &d.lm_chunk, make_lm_chunks(pl)))
    return -1;
  return 0;
}

// The "from the observation" form of the grouped pairs (ba_device.h PairObs), taken by a slim
// handle whose groups are all 32 wide and none of them masked, outside streaming (the chunk
// handles of ba_stream.hip keep the slim form).  Builds and uploads one PairObs per
// k_lin_grp piece and per k_schur_grp workgroup from lin_desc / grp_pat; a plan the side
// arrays cannot describe keeps the slim form.
int choose_pair_obs(ba_handle *h) {
  const ba::Plan &pl = h->plan;
  ba::DevProblem &d = h->d;
  d.pair_obs = 0;
  if (!d.pair_slim || !h->knobs.layout.pair_obs || h->arena || !pl.grp64.empty() || !pl.grp128.empty() ||
      pl.n_lin_plain != (int)pl.lin_desc.size() || pl.grp32.empty())
    return 0;
  std::vector<ba::PairObs> lin_obs(pl.lin_desc.size()), grp_obs(pl.grp32.size());
  std::vector<int> by_l0(pl.lin_desc.size());
  for (size_t k = 0; k < pl.lin_desc.size(); ++k) {
    const auto &g = pl.lin_desc[k];
    if (g.d > ba::kPairObsPoses || g.no > 255) return 0;
    ba::PairObs &po = lin_obs[k];
    po.o0 = g.o0;
    po.no = g.no;
    for (int jj = 0; jj < ba::kPairObsPoses; ++jj) po.sc[jj] = -1;
    for (int oo = 0; oo < g.no; ++oo) {
      const int y = pl.grp_pat[2 * ((size_t)g.pat0 + oo) + 1];
      if (!((y >> 30) & 1)) continue;  // (last writer of its pair: the last slot of an optimisable pose)
      const int jj = (y >> 16) & 0xff;
      if (jj >= g.d) return 0;
      po.sc[jj] = oo | (y & 0xffff) << 8;
    }
    for (int jj = 0; jj < ba::kPairObsPoses; ++jj) {
      if (jj < g.d && po.sc[jj] < 0) return 0;
      if (jj >= g.d) po.sc[jj] = 0;
    }
    by_l0[k] = (int)k;
  }
  std::sort(by_l0.begin(), by_l0.end(), [&](int a, int b) { return pl.lin_desc[a].l0 < pl.lin_desc[b].l0; });
  // the piece that holds landmark l, or -1
  auto piece_of = [&](int l) {
    auto it = std::upper_bound(by_l0.begin(), by_l0.end(), l, [&](int v, int k) { return v < pl.lin_desc[k].l0; });
    if (it == by_l0.begin()) return -1;
    const int k = *(it - 1);
    return l < pl.lin_desc[k].l0 + pl.lin_desc[k].nl ? k : -1;
  };
  for (size_t k = 0; k < pl.grp32.size(); ++k) {
    // a k_schur_grp workgroup lies inside ONE group: its first and last landmark are in pieces
    // of the same pattern whose observations are one run
    const auto &g = pl.grp32[k];
    const int ka = piece_of(g.l0), kb = piece_of(g.l0 + g.nl - 1);
    if (ka < 0 || kb < 0) return 0;
    const auto &a = pl.lin_desc[ka], &b = pl.lin_desc[kb];
    if (a.pat0 != b.pat0 || a.d != g.d || a.no != b.no || g.p0 != a.p0 + (int64_t)(g.l0 - a.l0) * a.d ||
        b.o0 != a.o0 + (int64_t)(b.l0 - a.l0) * a.no)
      return 0;
    grp_obs[k] = lin_obs[ka];
    grp_obs[k].o0 = a.o0 + (int64_t)(g.l0 - a.l0) * a.no;
  }
  static_assert(sizeof(ba::PairObs) == 32, "side array layout");
  if (h->upload(Mem::ChunkConst, &d.lin_obs, lin_obs.data(), lin_obs.size()) ||
      h->upload(Mem::ChunkConst, &d.grp_obs, grp_obs.data(), grp_obs.size()))
    return -1;
  d.pair_obs = 1;
  return 0;
}

// Structure, second half: the descriptors of super-runs, chunks and covisibility groups
// and the slot partials that go with them.
int upload_descriptors_and_groups(ba_handle *h) {
  const ba::Plan &pl = h->plan;
  ba::DevProblem &d = h->d;
  d.n_sup = (int)pl.sup_desc.size();
  d.n_bchunk = (int)pl.bchunk_lm.size() - 1;
  d.n_slot = (int)pl.slot_blk.size();
  static_assert(sizeof(ba::Plan::SupDesc) == sizeof(ba::DevProblem::SupDesc), "desc layout");
  static_assert(sizeof(ba::Plan::ChunkDesc) == sizeof(ba::DevProblem::ChunkDesc), "desc layout");
  static_assert(sizeof(ba::Plan::GrpDesc) == sizeof(ba::DevProblem::GrpDesc) && sizeof(ba::Plan::GrpDesc) == 128,
                "group descriptor layout");
  static_assert(sizeof(ba::Plan::LinDesc) == sizeof(ba::DevProblem::LinDesc) && sizeof(ba::Plan::LinDesc) == 48,
                "group linearisation descriptor layout");
  d.n_grp32 = (int)pl.grp32.size();
  d.n_grp64 = (int)pl.grp64.size();
  d.n_grp128 = (int)pl.grp128.size();
  // k_lin_grp: observation patterns, pose-side partial sums of the group pieces
  d.lin_chunk0 = pl.lin_groups ? pl.n_bchunk_grp : 0;
  d.n_lin_desc = (int)pl.lin_desc.size();
  d.n_lin_plain = pl.n_lin_plain;
  d.n_bs_grp = d.n_lin_desc;
  d.n_lm_part = d.n_bs_grp + (d.n_bchunk - d.lin_chunk0 + ba::kBsChunks - 1) / ba::kBsChunks;
  d.n_lin_cost = d.n_bchunk + d.n_lin_desc;
  // the grouped pairs — the first lm_pair_ptr[M_grp] — keep the slim record {G, w} when all
  // three group kernels handle them: k_lin_grp writes, k_schur_grp and the group role of
  // k_backsub_update read (ba_device.h kWSlim)
  d.pair_slim = h->knobs.layout.pair_slim && pl.lin_groups && d.n_lin_desc > 0 ? 1 : 0;
  d.P_slim = d.pair_slim ? pl.lm_pair_ptr[pl.M_grp] : 0;
  if (choose_pair_obs(h)) return -1;
  if (h->upload(Mem::ChunkConst, &d.sup_desc, pl.sup_desc.data(), pl.sup_desc.size()) ||
      h->upload(Mem::ChunkConst, &d.chunk_desc, pl.chunk_desc.data(), pl.chunk_desc.size()) ||
      h->dalloc(Mem::ChunkState, &d.spart2, (size_t)d.n_slot * ba::kSlotStride) ||
      h->upload(Mem::ChunkConst, &d.grp32, pl.grp32.data(), pl.grp32.size()) ||
      h->upload(Mem::ChunkConst, &d.grp64, pl.grp64.data(), pl.grp64.size()) ||
      h->upload(Mem::ChunkConst, &d.grp128, pl.grp128.data(), pl.grp128.size()) ||
      h->upload(Mem::ChunkConst, &d.lin_desc, pl.lin_desc.data(), pl.lin_desc.size()) ||
      h->upload(Mem::ChunkConst, &d.grp_pat, pl.grp_pat.data(), pl.grp_pat.size() / 2) ||  // (2 ints per slot)
      h->upload(Mem::ChunkConst, &d.pose_gpart_ptr, pl.pose_gpart_ptr) ||
      h->upload(Mem::ChunkConst, &d.pose_gpart, pl.pose_gpart) ||
      h->dalloc(Mem::ChunkState, &d.Apart2, (size_t)pl.n_apart2 * 27) ||
      h->dalloc(Mem::ChunkState, &d.lin_dump, (size_t)ba::kLinDump))
    return -1;
  if (pl.n_apart2 > 0) HIP_TRY(hipMemset(d.Apart2, 0, (size_t)pl.n_apart2 * 27 * sizeof(double)));
  return 0;
}

// Per-iteration storage: both block buffers, the landmark-side and pose-side scratch, the
// solution, the partial sums, the controller and its iteration log.
int alloc_iteration_storage(ba_handle *h) {
  const ba::Plan &pl = h->plan;
  ba::DevProblem &d = h->d;
  for (int k = 0; k < 2; ++k) {
    if (h->dalloc(Mem::ChunkState, &d.Cu[k], (size_t)pl.M * 6) || h->dalloc(Mem::ChunkState, &d.b[k], (size_t)pl.M * 3) ||
        h->dalloc(Mem::ChunkState, &d.W[k], std::max<size_t>(2, (size_t)pl.P * ba::kWStride)) ||
        h->dalloc(Mem::Resident, &d.A[k], (size_t)pl.N * 36) || h->dalloc(Mem::Resident, &d.a[k], (size_t)pl.N * 6))
      return -1;
    HIP_TRY(hipMemset(d.W[k], 0, std::max<size_t>(1, (size_t)pl.P * ba::kWStride) * sizeof(double)));
    HIP_TRY(hipMemset(d.A[k], 0, std::max<size_t>(1, (size_t)pl.N * 36) * sizeof(double)));
    HIP_TRY(hipMemset(d.a[k], 0, std::max<size_t>(1, (size_t)pl.N * 6) * sizeof(double)));
  }
  d.n_obs_lm = pl.M > 0 ? pl.lm_obs_ptr[pl.M] : 0;
  if (h->dalloc(Mem::ChunkState, &d.Cd, (size_t)pl.M * 6) || h->dalloc(Mem::ChunkState, &d.Cinv, (size_t)pl.M * 6) ||
      h->dalloc(Mem::ChunkState, &d.lin_cost_part, (size_t)std::max(1, d.n_lin_cost)) ||
      h->dalloc(Mem::ChunkState, &d.Apart, (size_t)d.n_achunk * 27) ||
      h->dalloc(Mem::ChunkState, &d.spart, (size_t)d.n_tchunk * ba::kSlotStride) ||
      h->dalloc(Mem::ChunkState, &d.y, (size_t)pl.M * 3) ||
      h->dalloc(Mem::ChunkState, &d.lm_part, (size_t)std::max(1, d.n_lm_part) * 2))
    return -1;
  d.log_cap = 4096;
  if (h->dalloc(Mem::Resident, &d.x, (size_t)pl.N * 6 + 64) ||
      h->dalloc(Mem::Resident, &d.cost_part, (size_t)ba::kCostGrid) ||
      h->dalloc(Mem::Resident, &d.pose_part, (size_t)2 + 2 * ba::kPoseGrid) ||
      h->dalloc(Mem::Resident, &d.scal, (size_t)4) || h->dalloc(Mem::Resident, &d.ctrl, (size_t)1) ||
      h->dalloc(Mem::Resident, &d.log, (size_t)d.log_cap))
    return -1;
  HIP_TRY(hipMemset(d.lin_cost_part, 0, (size_t)std::max(1, d.n_lin_cost) * sizeof(double)));
  HIP_TRY(hipMemset(d.x, 0, ((size_t)pl.N * 6 + 64) * sizeof(double)));
  HIP_TRY(hipMemset(d.y, 0, std::max<size_t>(1, (size_t)pl.M * 3) * sizeof(double)));
  HIP_TRY(hipMemset(d.cost_part, 0, ba::kCostGrid * sizeof(double)));
  HIP_TRY(hipMemset(d.lm_part, 0, (size_t)std::max(1, d.n_lm_part) * 2 * sizeof(double)));
  HIP_TRY(hipMemset(d.pose_part, 0, (2 + 2 * ba::kPoseGrid) * sizeof(double)));
  HIP_TRY(hipMemset(d.scal, 0, 4 * sizeof(double)));
  return 0;
}

// Streaming (ba_stream.hip): the reduced system is scattered, factorised and solved ONCE
// per iteration, by the owner; this handle aliases its dense image, schedule and solution
// (the S-block numbering and the tile schedule are global: identical on every landmark
// chunk) and keeps only its own packed partial S||rhs.
int alias_dense_owner(ba_handle *h) {
  const ba_handle *o = h->dense_owner;
  ba::DevProblem &d = h->d;
  if (!o->finalized || o->plan.N != h->plan.N || o->plan.B != h->plan.B)
    return fail("ba_finalize: the dense owner belongs to a different problem");
  h->sched = o->sched;
  h->ddev = o->ddev;
  h->pose_col_h = o->pose_col_h;
  d.nb = o->d.nb; d.npad = o->d.npad; d.ld = o->d.ld;
  d.L = o->d.L; d.Ldiag = o->d.Ldiag; d.pose_col = o->d.pose_col; d.col_x = o->d.col_x;
  d.zt_I = o->d.zt_I; d.zt_J = o->d.zt_J; d.n_zt = o->d.n_zt;
  d.x = o->d.x;
  return 0;
}

// The dense reduced system of this handle: tiles of 5 poses (32 columns) or 10 poses (64
// columns), eliminated in the order of the level schedule.  Both schedules are built;
// dense_pick_tile_order chooses.  Then the image, the schedule's device lists and the
// lists of the tiles that every iteration resets.
int build_dense_system(ba_handle *h) {
  const ba::Plan &pl = h->plan;
  ba::DevProblem &d = h->d;
  const ba::DenseKnobs &knobs = h->knobs.dense;
  ba::DenseSchedule cand[2];
  const int orders[2] = {32, 64};
  for (int k = 0; k < 2; ++k) {
    int ncb_k = 0;
    std::vector<uint8_t> adj;
    ba::tile_pattern(pl, ba::dense_poses_per_tile(orders[k]), ncb_k, adj);
    if (knobs.full) std::fill(adj.begin(), adj.end(), 1);
    ba::build_dense_schedule(ncb_k, adj, knobs.natural, orders[k], cand[k], knobs.order);
  }
  const bool stats = h->knobs.plan.stats;
  if (stats)
    fprintf(stderr, "dense schedules: nb32 %d tiles %d levels max_rows %d fill %.3f | nb64 %d tiles %d levels max_rows %d fill %.3f\n",
            cand[0].ncb, cand[0].nlev, cand[0].max_rows, cand[0].fill, cand[1].ncb, cand[1].nlev, cand[1].max_rows,
            cand[1].fill);
  h->sched = cand[ba::dense_pick_tile_order(cand[0], cand[1], knobs.nb)];
  const ba::DenseSchedule &sc = h->sched;
  ba::DenseDev &dd = h->ddev;
  const int nb = sc.nb;
  const int ppt = ba::dense_poses_per_tile(nb);
  const int ncb = sc.ncb;
  d.nb = nb;
  d.npad = ncb * nb;
  d.ld = d.npad + nb;
  if (h->dalloc(Mem::Resident, &d.L, (size_t)d.npad * d.ld) ||
      h->dalloc(Mem::Resident, &d.Ldiag, (size_t)ncb * ba::dense_ws_per_block(nb)))
    return -1;
  h->pose_col_h.assign(pl.N, 0);
  std::vector<int> col_x((size_t)d.npad, -1);
  for (int j = 0; j < pl.N; ++j) {
    const int c0 = sc.pos_of_tile[j / ppt] * nb + 6 * (j % ppt);
    h->pose_col_h[j] = c0;
    for (int r = 0; r < 6; ++r) col_x[c0 + r] = 6 * j + r;
  }
  if (h->upload(Mem::Resident, &d.pose_col, h->pose_col_h) || upload_dense_schedule(h, sc, col_x, dd)) return -1;
  d.col_x = dd.col_x;
  if (h->knobs.plan.times && dd.dag_items) fprintf(stderr, "[finalize] k_chol_dag: %d items\n", dd.plan[1].n_dag_items);
  if (stats) {
    fprintf(stderr, "dense launch plan: nb%d forward %s backward %s tail %d columns%s\n", nb,
            ba::dense_fwd_name(dd.plan[1].fwd), ba::dense_back_name(dd.plan[1].back), dd.plan[1].tail_cols,
            dd.plan[1].tail_pair ? " (pair)" : "");
    fprintf(stderr, "dense cone sweep: %s (%d leaves, longest cone %d, %d steps for %d non-tail tiles, max_rows %d)\n",
            dd.plan[1].back_cone ? "taken instead" : "not taken", dd.plan[1].cone_leaves, dd.plan[1].cone_max,
            dd.plan[1].cone_steps, dd.plan[1].back_t_end, sc.max_rows);
  }
  // tiles (re)initialised per iteration: factor pattern + diagonal + rhs row
  std::vector<int> ztI, ztJ;
  for (int p = 0; p < ncb; ++p) {
    ztI.push_back(p);
    ztJ.push_back(p);
    for (int q = sc.row_ptr[p]; q < sc.row_ptr[p + 1]; ++q) {
      ztI.push_back(sc.rows[q]);  // includes the rhs row block (== ncb)
      ztJ.push_back(p);
    }
  }
  d.n_zt = (int)ztI.size();
  if (h->upload(Mem::Resident, &d.zt_I, ztI) || h->upload(Mem::Resident, &d.zt_J, ztJ)) return -1;
  HIP_TRY(hipMemset(d.L, 0, (size_t)d.npad * d.ld * sizeof(double)));
  return 0;
}

// The packed partial S||rhs (exchange buffer 0) and the dense reduced system behind it.
int setup_reduced_system(ba_handle *h) {
  const ba::Plan &pl = h->plan;
  h->xbuf_n[0] = pl.B * 36 + 6 * (int64_t)pl.N;
  h->xbuf_n[1] = 4;
  h->xbuf_n[2] = 3 * (int64_t)pl.n_pt_global;
  if (h->dalloc(Mem::Resident, &h->d.Spk, (size_t)h->xbuf_n[0])) return -1;
  HIP_TRY(hipMemset(h->d.Spk, 0, (size_t)h->xbuf_n[0] * sizeof(double)));
  return h->dense_owner ? alias_dense_owner(h) : build_dense_system(h);
}

// The relative-pose factors (ba_set_relative): the planner's lists, the packed values and
// both scratch buffers.  Pose-sized and read while no chunk is resident: Resident.
int upload_relative(ba_handle *h) {
  const ba::Plan &pl = h->plan;
  ba::RelDev &r = h->rel;
  r = ba::RelDev{};
  h->rel_bytes = 0;
  const size_t F = (size_t)pl.n_rel;
  if (F == 0) return 0;
  constexpr Mem R = Mem::Resident;
  static_assert(sizeof(int4) == 16, "layout");
  int4 *jk = nullptr;
  double *val = nullptr;
  int32_t *pptr = nullptr, *plist = nullptr, *blk = nullptr, *bptr = nullptr, *blist = nullptr;
  const int n_part = (int)((F + ba::kRelFpb - 1) / ba::kRelFpb);
  if (h->upload(R, &jk, pl.rel_jk.data(), F) || h->upload(R, &val, h->rel_val) || h->upload(R, &pptr, pl.rel_pptr) ||
      h->upload(R, &plist, pl.rel_plist) || h->upload(R, &blk, pl.rel_blk) || h->upload(R, &bptr, pl.rel_bptr) ||
      h->upload(R, &blist, pl.rel_blist) || h->dalloc(R, &r.scr[0], F * ba::kRelScr) ||
      h->dalloc(R, &r.scr[1], F * ba::kRelScr) || h->dalloc(R, &r.part, (size_t)2 * n_part))
    return -1;
  for (int k = 0; k < 2; ++k) HIP_TRY(hipMemset(r.scr[k], 0, F * ba::kRelScr * sizeof(double)));
  HIP_TRY(hipMemset(r.part, 0, (size_t)2 * n_part * sizeof(double)));
  r.F = (int)F;
  r.nblk = (int)pl.rel_blk.size();
  r.n_part = n_part;
  r.jk = jk;
  r.val = val;
  r.pptr = pptr;
  r.plist = plist;
  r.blk = blk;
  r.bptr = bptr;
  r.blist = blist;
  h->rel_bytes = F * (16 + ba::kRelVal * 8 + 2 * ba::kRelScr * 8) + (pl.rel_pptr.size() + pl.rel_plist.size() +
                 pl.rel_blk.size() + pl.rel_bptr.size() + pl.rel_blist.size()) * 4 + (size_t)2 * n_part * 8;
  return 0;
}

// why a handle that holds relative-pose factors cannot be sharded (ba_set_shard,
// ba_set_allreduce, ba_set_relative: whichever comes second is refused)
const char *kRelNoShard = "relative-pose factors run on one GPU: a handle that holds them cannot be sharded "
                          "(ba_set_shard with world > 1, or an all-reduce hook)";

}  // namespace

extern "C" {

const char *ba_last_error(void) { return g_err.c_str(); }

int ba_create(ba_handle **out, int device_id) {
  if (!out) return fail("ba_create: null out pointer");
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0)
    return fail("ba_create: no HIP device available (the HIP path has no CPU "
                "fallback)");
  if (device_id < 0 || device_id >= ndev) return fail("ba_create: bad device id");
  ba_handle *h = new ba_handle();
  h->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess ||
      hipStreamCreate(&h->own_stream) != hipSuccess ||
      hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) {
    delete h;
    return fail("ba_create: cannot create stream");
  }
  h->stream = h->own_stream;
  h->knobs = ba::Knobs::from_env();
  h->overlap = h->knobs.run.overlap;
  h->use_graph = h->knobs.run.graph;
  std::memset(&h->d, 0, sizeof(h->d));
  std::memset(&h->hc, 0, sizeof(h->hc));
  *out = h;
  return 0;
}

void ba_destroy(ba_handle *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  h->free_device();
  for (hipEvent_t e : h->kt.pool) (void)hipEventDestroy(e);
  h->kt.pool.clear();
  if (h->ev_ok)
    for (int k = 0; k <= ST_N; ++k) (void)hipEventDestroy(h->ev[k]);
  h->drop_graph();
  if (h->side_stream) {
    (void)hipStreamSynchronize(h->side_stream);
    (void)hipStreamDestroy(h->side_stream);
  }
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
}

int ba_set_stream(ba_handle *h, void *hip_stream) {
  if (!h) return fail("null handle");
  h->drop_graph();
  // the given value is used as is: NULL is HIP's (legacy) default stream, which
  // is also what torch.cuda.current_stream().cuda_stream reports by default
  h->stream = (hipStream_t)hip_stream;
  return 0;
}

int ba_set_cameras(ba_handle *h, int n_cam, const double *intr4,
                   const double *T_cj12) {
  if (!h || n_cam <= 0 || !intr4 || !T_cj12) return fail("ba_set_cameras: bad argument");
  if (h->finalized) return fail("ba_set_cameras: already finalized");
  h->n_cam = n_cam;
  h->cam_intr.assign(intr4, intr4 + 4 * (size_t)n_cam);
  h->cam_T.assign(T_cj12, T_cj12 + 12 * (size_t)n_cam);
  return 0;
}

int ba_set_poses(ba_handle *h, int n_pose, const double *T_jw12,
                 const uint8_t *fixed) {
  if (!h || n_pose <= 0 || !T_jw12) return fail("ba_set_poses: bad argument");
  if (h->finalized) return fail("ba_set_poses: already finalized");
  h->n_pose = n_pose;
  h->pose_T.assign(T_jw12, T_jw12 + 12 * (size_t)n_pose);
  if (fixed)
    h->pose_fixed.assign(fixed, fixed + n_pose);
  else
    h->pose_fixed.assign(n_pose, 0);
  return 0;
}

int ba_set_points(ba_handle *h, int n_pt, const double *X3,
                  const uint8_t *fixed) {
  if (!h || n_pt <= 0 || !X3) return fail("ba_set_points: bad argument");
  if (h->finalized) return fail("ba_set_points: already finalized");
  h->n_pt = n_pt;
  h->pt_X.assign(X3, X3 + 3 * (size_t)n_pt);
  if (fixed)
    h->pt_fixed.assign(fixed, fixed + n_pt);
  else
    h->pt_fixed.assign(n_pt, 0);
  return 0;
}

int ba_set_observations(ba_handle *h, int64_t n_obs, const int32_t *cam,
                        const int32_t *pose, const int32_t *point,
                        const double *uv2) {
  if (!h || n_obs < 0 || (n_obs > 0 && (!cam || !pose || !point || !uv2)))
    return fail("ba_set_observations: bad argument");
  if (h->finalized) return fail("ba_set_observations: already finalized");
  h->n_obs = n_obs;
  h->obs_cam.assign(cam, cam + n_obs);
  h->obs_pose.assign(pose, pose + n_obs);
  h->obs_pt.assign(point, point + n_obs);
  h->obs_uv.assign(uv2, uv2 + 2 * n_obs);
  return 0;
}

int ba_set_shard(ba_handle *h, int rank, int world) {
  if (!h || world < 1 || rank < 0 || rank >= world) return fail("ba_set_shard: bad argument");
  if (h->finalized) return fail("ba_set_shard: already finalized");
  if (world > 1 && !h->rel_j.empty()) return fail(std::string("ba_set_shard: ") + kRelNoShard);
  h->rank = rank;
  h->world = world;
  return 0;
}

int ba_relative_check(int n_pose, const uint8_t *pose_fixed, int64_t n_rel, const int32_t *rel_j,
                      const int32_t *rel_k, const double *Z12, const double *Omega36) {
  std::string err;
  if (ba::relative_validate_host(ba::kRelPairs | ba::kRelValues, n_pose, pose_fixed, n_rel, rel_j, rel_k, Z12,
                                 Omega36, &err))
    return fail("ba_relative_check: " + err);
  return 0;
}

int ba_set_relative(ba_handle *h, int64_t n_rel, const int32_t *rel_j, const int32_t *rel_k, const double *Z12,
                    const double *Omega36) {
  if (!h) return fail("ba_set_relative: null handle");
  if (h->finalized) return fail("ba_set_relative: already finalized (the factors change the structure; "
                                "ba_update_relative takes new values for the same pairs)");
  if (n_rel == 0 || (!rel_j && !rel_k && !Z12 && !Omega36)) {
    h->rel_j.clear();
    h->rel_k.clear();
    h->rel_val.clear();
    return 0;
  }
  if (h->arena || h->dense_owner) return fail("ba_set_relative: not available on a streamed chunk");
  if (h->world > 1 || h->ar_fn) return fail(std::string("ba_set_relative: ") + kRelNoShard);
  if (h->use_graph)
    return fail("ba_set_relative: BA_GRAPH=1 replay is not available with relative-pose factors");
  if (h->n_pose <= 0) return fail("ba_set_relative: the poses must be set first (ba_set_poses)");
  std::string err;
  if (ba::relative_validate_host(ba::kRelPairs | ba::kRelValues, h->n_pose, h->pose_fixed.data(), n_rel, rel_j, rel_k,
                                 Z12, Omega36, &err))
    return fail("ba_set_relative: " + err);
  h->rel_j.assign(rel_j, rel_j + n_rel);
  h->rel_k.assign(rel_k, rel_k + n_rel);
  ba::relative_pack_values(n_rel, Z12, Omega36, &h->rel_val);
  return 0;
}

int ba_update_relative(ba_handle *h, const double *Z12, const double *Omega36) {
  if (!h || !h->finalized) return fail("ba_update_relative: not finalized");
  if (h->rel.F <= 0) return fail("ba_update_relative: the handle holds no relative-pose factors (ba_set_relative)");
  std::string err;
  if (ba::relative_validate_host(ba::kRelValues, h->n_pose, nullptr, h->rel.F, nullptr, nullptr, Z12, Omega36, &err))
    return fail("ba_update_relative: " + err);
  if (use_device(h)) return -1;
  join_side(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  ba::relative_pack_values(h->rel.F, Z12, Omega36, &h->rel_val);
  HIP_TRY(hipMemcpy(const_cast<double *>(h->rel.val), h->rel_val.data(), h->rel_val.size() * sizeof(double),
                    hipMemcpyHostToDevice));
  h->lm_begun = false;  // the blocks on the device belong to the old values: ba_lm_begin linearises again
  h->tiles_ready = false;
  return 0;
}

int ba_relative_info(ba_handle *h, int64_t out4[4]) {
  if (!h || !out4) return fail("ba_relative_info: bad argument");
  out4[0] = (int64_t)h->rel_j.size();
  out4[1] = h->finalized ? (int64_t)h->plan.rel_blk.size() : 0;
  out4[2] = h->finalized ? h->plan.n_rel_only : 0;
  out4[3] = h->finalized ? (int64_t)h->rel_bytes : 0;
  return 0;
}

int ba_partition_points(int n_pose, const uint8_t *pose_fixed, int n_pt,
                        const uint8_t *pt_fixed, int64_t n_obs,
                        const int32_t *obs_pose, const int32_t *obs_pt,
                        int world, int32_t *owner_out) {
  if (n_pose <= 0 || n_pt <= 0 || world < 1 || !owner_out)
    return fail("ba_partition_points: bad argument");
  std::vector<uint8_t> pf(n_pose, 0), qf(n_pt, 0);
  ba::PlanInput in;
  in.n_cam = 1;
  in.n_pose = n_pose;
  in.pose_fixed = pose_fixed ? pose_fixed : pf.data();
  in.n_pt = n_pt;
  in.pt_fixed = pt_fixed ? pt_fixed : qf.data();
  in.n_obs = n_obs;
  in.obs_pose = obs_pose;
  in.obs_pt = obs_pt;
  in.world = world;
  for (int64_t k = 0; k < n_obs; ++k)
    if (obs_pose[k] < 0 || obs_pose[k] >= n_pose || obs_pt[k] < 0 || obs_pt[k] >= n_pt)
      return fail("ba_partition_points: observation index out of range");
  std::vector<int32_t> owner;
  ba::partition_points(in, ba::Knobs::from_env().plan.threads, owner);  // (no handle: read per call)
  std::memcpy(owner_out, owner.data(), sizeof(int32_t) * (size_t)n_pt);
  return 0;
}

int ba_finalize(ba_handle *h) {
  if (h) h->drop_graph();
  if (!h) return fail("null handle");
  if (h->finalized) return 0;  // idempotent (README of the reference calls it publicly)
  if (h->n_cam <= 0 || h->n_pose <= 0 || h->n_pt <= 0)
    return fail("ba_finalize: cameras, poses and points must be set first");
  if (use_device(h)) return -1;
  const bool times = h->knobs.plan.times;
  h->up_alloc_s = h->up_copy_s = 0;
  h->up_bytes = h->up_calls = 0;
  auto t_last = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) {
    if (!times) return;
    (void)hipDeviceSynchronize();
    const auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "[finalize] %-26s %7.1f ms   (uploads so far: %zu calls, %.1f MB, alloc %.1f ms, copy %.1f ms)\n", what,
            std::chrono::duration<double, std::milli>(n - t_last).count(), h->up_calls, h->up_bytes / 1e6,
            h->up_alloc_s * 1e3, h->up_copy_s * 1e3);
    t_last = n;
  };
  if (!h->rel_j.empty()) {
    // the poses may have been set again since ba_set_relative: no index reaches the planner
    // or a kernel unchecked
    std::string err;
    if (ba::relative_validate_host(ba::kRelPairs, h->n_pose, h->pose_fixed.data(), (int64_t)h->rel_j.size(),
                                   h->rel_j.data(), h->rel_k.data(), nullptr, nullptr, &err))
      return fail("ba_finalize: relative-pose factors: " + err);
    if (h->world > 1 || h->ar_fn) return fail(std::string("ba_finalize: ") + kRelNoShard);
  }
  if (finalize_plan(h)) return -1;
  lap("host plan");
  if (upload_parameters(h) || upload_observation_lists(h) || upload_descriptors_and_groups(h)) return -1;
  lap("structure uploads");
  if (alloc_iteration_storage(h)) return -1;
  lap("block storage");
  if (setup_reduced_system(h)) return -1;
  lap("dense schedule + image");
  if (upload_relative(h)) return -1;
  std::memset(&h->hc, 0, sizeof(h->hc));
  h->hc.lambda = 100.0;
  h->hc.huber = 1.0;
  h->hc.max_iter = 1;
  HIP_TRY(hipMemcpy(h->d.ctrl, &h->hc, sizeof(ba::DevCtrl), hipMemcpyHostToDevice));
  HIP_TRY(hipDeviceSynchronize());
  h->finalized = true;
  return 0;
}

int ba_update_values(ba_handle *h, const double *T_jw12, const double *X3) {
  if (!h || !h->finalized) return fail("ba_update_values: not finalized");
  if (h->arena) return fail("ba_update_values: not available on a streamed chunk");
  if (use_device(h)) return -1;
  const ba::Plan &pl = h->plan;
  join_side(h);
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (T_jw12) {
    h->pose_T.assign(T_jw12, T_jw12 + 12 * (size_t)pl.n_pose);
    std::vector<double> poses((size_t)pl.n_pose * 12);
    for (int p = 0; p < pl.n_pose; ++p)
      std::memcpy(&poses[(size_t)p * 12], T_jw12 + (size_t)pl.pose_user_of_int[p] * 12, 12 * sizeof(double));
    for (int k = 0; k < 2; ++k)
      HIP_TRY(hipMemcpy(h->d.poses[k], poses.data(), poses.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (X3) {
    h->pt_X.assign(X3, X3 + 3 * (size_t)pl.n_pt_global);
    std::vector<double> pts((size_t)pl.n_pt * 3);
    for (int q = 0; q < pl.n_pt; ++q)
      std::memcpy(&pts[(size_t)q * 3], X3 + (size_t)pl.pt_user_of_int[q] * 3, 3 * sizeof(double));
    if (pl.n_pt > 0)
      for (int k = 0; k < 2; ++k)
        HIP_TRY(hipMemcpy(h->d.pts[k], pts.data(), pts.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  h->gathered_valid = false;
  h->lm_begun = false;   // the blocks on the device belong to the old values: ba_lm_begin linearises again
  h->gd_begun = false;   // (the GD index stays: it depends on the structure only)
  h->tiles_ready = false;
  return 0;
}

int ba_set_allreduce(ba_handle *h, ba_allreduce_fn fn, void *user) {
  if (!h) return fail("null handle");
  if (fn && !h->rel_j.empty()) return fail(std::string("ba_set_allreduce: ") + kRelNoShard);
  h->ar_fn = fn;
  h->ar_user = user;
  return 0;
}

int64_t ba_reduce_buffer_size(ba_handle *h, int which) {
  if (!h || !h->finalized || which < 0 || which > 2) return -1;
  return h->xbuf_n[which];
}

int ba_bind_reduce_buffer(ba_handle *h, int which, void *dev_ptr, int64_t n) {
  if (!h || !h->finalized) return fail("ba_bind_reduce_buffer: not finalized");
  h->drop_graph();
  if (which < 0 || which > 2 || !dev_ptr || n < h->xbuf_n[which])
    return fail("ba_bind_reduce_buffer: bad argument");
  if (which == 0)
    h->d.Spk = (double *)dev_ptr;
  else if (which == 1)
    h->d.scal = (double *)dev_ptr;
  else {
    h->gbuf = (double *)dev_ptr;  // (a buffer of the library's own stays in `allocs`)
    h->gbuf_bound = true;
  }
  return 0;
}

// ---------------------------------------------------------------------------
}  // extern "C"

// Controller state for a new LM loop (reference :705-708): everything of
// ba_lm_begin but the first linearisation.  *done_after = the loop is over before it
// starts (max_num_iterations <= 0).  Shared with ba_stream.hip.
int ba::lm_prepare_ctrl(ba_handle *h, const ba_options *opt, int *done_after) {
  if (opt->max_num_iterations > h->d.log_cap) {
    // grow the device-side iteration log.  k_control writes it while no chunk of a
    // streamed problem is resident: Resident, like the log it replaces
    ba::DevIterRec *nl = nullptr;
    if (h->dalloc(Mem::Resident, &nl, (size_t)opt->max_num_iterations)) return -1;
    h->drop_graph();  // the captured kernels hold the old pointer
    h->d.log = nl;
    h->d.log_cap = opt->max_num_iterations;
  }
  h->tiles_ready = false;
  h->gathered_valid = false;
  if (pull_ctrl(h)) return -1;  // keep `cur` and `lcur`
  ba::DevCtrl &c = h->hc;
  c.lambda = (double)opt->initial_lambda;
  c.huber = (double)opt->threshold_huber_loss;
  c.thr_step = (double)opt->threshold_step_size;
  c.thr_cost = (double)opt->threshold_cost_change;
  c.dec_ratio = (double)opt->decrease_ratio_lambda;
  c.inc_ratio = (double)opt->increase_ratio_lambda;
  c.max_iter = opt->max_num_iterations;
  c.gn = opt->gauss_newton ? 1 : 0;
  c.iter = 0;
  c.converged = 0;
  c.prev_cost = 0.0;
  *done_after = (opt->max_num_iterations <= 0) ? 1 : 0;
  c.done = 0;
  if (push_ctrl(h)) return -1;
  HIP_TRY(hipMemsetAsync(h->ddev.bad_pivots, 0, sizeof(int), h->stream));
  return 0;
}
int ba::ctrl_pull(ba_handle *h) { return pull_ctrl(h); }
int ba::ctrl_push(ba_handle *h) { return push_ctrl(h); }

extern "C" {

int ba_lm_begin(ba_handle *h, const ba_options *opt) {
  if (!h || !opt) return fail("ba_lm_begin: bad argument");
  if (!h->finalized && ba_finalize(h)) return -1;
  if (use_device(h)) return -1;
  join_side(h);
  int done_after = 0;
  if (ba::lm_prepare_ctrl(h, opt, &done_after)) return -1;
  h->gd_begun = false;
  // first linearisation, at the starting point; previous_cost =
  // EvaluateCurrentCost() (reference :707) is the sum of its residual norms
  enqueue_linearize(h, 0);
  const bool rel = h->rel.F > 0;
  if (rel) ba::launch_rel_lin(h->d, h->rel, 0, 1, h->stream);
  ba::launch_scalars_cost_only(h->d, 1, h->stream);
  if (rel) ba::launch_rel_gather(h->d, h->rel, 0, 3, h->stream);  // A_j, a_j and the cost gain the factors
  if (xchg(h, 1)) return -1;
  ba::launch_init_ctrl_cost(h->d, h->stream);
  if (done_after) {
    if (pull_ctrl(h)) return -1;
    h->hc.done = 1;
    if (push_ctrl(h)) return -1;
  }
  HIP_TRY(hipGetLastError());
  h->lm_begun = true;
  return 0;
}

int ba_lm_iterate(ba_handle *h, int n) {
  if (h && !h->lm_begun && h->gd_begun)
    return fail("ba_lm_iterate: the handle is in a gradient-descent loop (ba_gd_begin); call ba_lm_begin first");
  if (!h || !h->lm_begun) return fail("ba_lm_iterate: call ba_lm_begin first");
  if (use_device(h)) return -1;
  h->gathered_valid = false;
  // Graph replay: the kernels early-exit on the device-side `done` word and
  // take the whole problem by value, so one captured iteration is valid until
  // the problem, the stream or the exchange buffers change (drop_graph()).
  const bool graphable = h->use_graph && !h->timing && !h->ar_fn && h->stream != nullptr;
  if (graphable && !h->graph_exec && n > 0) {
    HIP_TRY(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
    const int rc = enqueue_iteration(h);
    hipGraph_t g = nullptr;
    const hipError_t ec = hipStreamEndCapture(h->stream, &g);
    if (rc != 0 || ec != hipSuccess || !g) {
      if (g) (void)hipGraphDestroy(g);
      (void)hipGetLastError();
      h->use_graph = false;  // fall back to plain launches on this handle
    } else {
      h->graph = g;
      if (hipGraphInstantiate(&h->graph_exec, g, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        h->drop_graph();
        h->use_graph = false;
      }
    }
  }
  for (int k = 0; k < n; ++k) {
    if (graphable && h->graph_exec) {
      HIP_TRY(hipGraphLaunch(h->graph_exec, h->stream));
    } else if (enqueue_iteration(h)) {
      return -1;
    }
  }
  return 0;
}

int ba_lm_sync(ba_handle *h, ba_iter_info *out, int cap, int *n_iter,
               int *converged) {
  if (!h || !h->lm_begun) return fail("ba_lm_sync: call ba_lm_begin first");
  if (use_device(h)) return -1;
  if (h->side_pending) (void)hipStreamWaitEvent(h->stream, h->ev_join, 0);  // (stays pending: the
  //   next iteration joins it again, which is harmless)
  if (pull_ctrl(h)) return -1;
  {
    // A hand-off of a dataflow sweep of the reduced solve that timed out (bounded
    // polls, ba_dense_tile.inc) left x partly unsolved: the device added kFlowTimeout
    // to the pivot counter.  That is an ERROR of the solve, not a dropped pivot.
    int bp = 0;
    HIP_TRY(hipMemcpy(&bp, h->ddev.bad_pivots, sizeof(int), hipMemcpyDeviceToHost));
    if (bp >= ba::kFlowTimeout)
      return fail("ba_lm_sync: a dataflow hand-off of the reduced solve timed out (" +
                  std::to_string(bp / ba::kFlowTimeout) + " polls gave up); the iterations since ba_lm_begin "
                  "are invalid. BA_DENSE_FLOW=0 selects the per-level launches");
  }
  const int n = h->hc.iter;
  if (n_iter) *n_iter = n;
  if (converged) *converged = h->hc.converged;
  if (out && cap > 0 && n > 0) {
    static_assert(sizeof(ba::DevIterRec) == sizeof(ba_iter_info), "iter layout");
    const int m = std::min(std::min(n, cap), h->d.log_cap);
    HIP_TRY(hipMemcpy(out, h->d.log, (size_t)m * sizeof(ba_iter_info), hipMemcpyDeviceToHost));
  }
  return h->hc.done ? 1 : 0;  // 1 = loop finished
}

int ba_solve(ba_handle *h, const ba_options *opt, ba_iter_info *out, int cap,
             int *n_iter, int *converged) {
  if (ba_lm_begin(h, opt)) return -1;
  int done = opt->max_num_iterations <= 0;
  int issued = 0;
  while (!done) {
    const int batch = std::min(4, opt->max_num_iterations - issued);
    if (batch <= 0) break;
    if (ba_lm_iterate(h, batch)) return -1;
    issued += batch;
    int rc = ba_lm_sync(h, nullptr, 0, nullptr, nullptr);
    if (rc < 0) return -1;
    done = rc;
  }
  int rc = ba_lm_sync(h, out, cap, n_iter, converged);
  return rc < 0 ? -1 : 0;
}

// ---------------------------------------------------------------------------
// gradient descent, FullBundleAdjustmentSolverRefactor::SolveByGradientDescent
// (reference core/full_bundle_adjustment_solver_refactor.cpp:1075-1367)

// Device state of the GD loop, built once per ba_finalize on the first GD call: the
// pose-major index of every real observation of an optimisable pose (stable in the
// landmark-major order, padded slots left out), its chunks and the partial-sum arrays.
// The LM path's lists and buffers are not touched.
static int gd_prepare(ba_handle *h, const char *who) {
  if (h->world > 1 || h->ar_fn)
    return fail(std::string(who) + ": gradient descent runs on one GPU; this handle is sharded "
                "(ba_set_shard with world > 1, or an all-reduce hook is set)");
  if (h->rel.F > 0)
    return fail(std::string(who) + ": gradient descent takes reprojections only; this handle holds relative-pose "
                "factors (ba_set_relative)");
  if (h->gd_ready) return 0;
  const ba::Plan &pl = h->plan;
  const ba::DevProblem &d = h->d;
  const int N = pl.N;
  std::vector<int64_t> ptr((size_t)N + 1, 0);
  auto real = [&](int64_t s) { return pl.obs_uv[2 * s] == pl.obs_uv[2 * s]; };  // (uv = NaN: padded slot)
  for (int64_t s = 0; s < pl.n_obs; ++s) {
    const int j = pl.obs_idx[4 * s + 1];
    if (j < N && real(s)) ptr[j + 1]++;
  }
  for (int j = 0; j < N; ++j) ptr[j + 1] += ptr[j];
  const int64_t n = ptr[N];
  std::vector<int32_t> pobs((size_t)n * 2);
  std::vector<double> puv((size_t)n * 2);
  {
    std::vector<int64_t> cur(ptr.begin(), ptr.end() - 1);
    for (int64_t s = 0; s < pl.n_obs; ++s) {
      const int j = pl.obs_idx[4 * s + 1];
      if (j >= N || !real(s)) continue;
      const int64_t o = cur[j]++;
      pobs[2 * o + 0] = pl.obs_idx[4 * s + 0];  // camera
      pobs[2 * o + 1] = pl.obs_idx[4 * s + 2];  // point
      puv[2 * o + 0] = pl.obs_uv[2 * s + 0];
      puv[2 * o + 1] = pl.obs_uv[2 * s + 1];
    }
  }
  std::vector<int32_t> chunk_pose, pose_chunk_ptr((size_t)N + 1, 0);
  std::vector<int64_t> chunk_begin, chunk_end;
  for (int j = 0; j < N; ++j) {
    for (int64_t b = ptr[j]; b < ptr[j + 1]; b += ba::kGdChunk) {
      chunk_pose.push_back(j);
      chunk_begin.push_back(b);
      chunk_end.push_back(std::min<int64_t>(b + ba::kGdChunk, ptr[j + 1]));
    }
    pose_chunk_ptr[j + 1] = (int32_t)chunk_pose.size();
  }
  ba::GdDev &g = h->gd;
  g = ba::GdDev{};
  g.n_chunk = (int)chunk_pose.size();
  const int64_t n_fix = d.n_obs - d.n_obs_lm;
  g.n_fix_blk = n_fix > 0 ? (int)std::min<int64_t>(ba::kGdFixGrid, (n_fix + 255) / 256) : 0;
  g.n_cost_part = d.n_bchunk + g.n_fix_blk;
  g.n_upd_pose_blk = (N + 255) / 256;
  g.n_upd_blk = g.n_upd_pose_blk + (d.M + 255) / 256;
  static_assert(sizeof(int2) == 8 && sizeof(double2) == 16, "layout");
  if (h->upload(Mem::Resident, &g.pobs, pobs.data(), (size_t)n) ||
      h->upload(Mem::Resident, &g.puv, puv.data(), (size_t)n) ||
      h->upload(Mem::Resident, &g.chunk_pose, chunk_pose) || h->upload(Mem::Resident, &g.chunk_begin, chunk_begin) ||
      h->upload(Mem::Resident, &g.chunk_end, chunk_end) ||
      h->upload(Mem::Resident, &g.pose_chunk_ptr, pose_chunk_ptr) ||
      h->dalloc(Mem::Resident, &g.ppart, (size_t)g.n_chunk * 6) || h->dalloc(Mem::Resident, &g.a, (size_t)N * 6) ||
      h->dalloc(Mem::Resident, &g.b, (size_t)d.M * 3) ||
      h->dalloc(Mem::Resident, &g.cost_part, (size_t)g.n_cost_part) ||
      h->dalloc(Mem::Resident, &g.step_part, (size_t)g.n_upd_blk * 2))
    return -1;
  HIP_TRY(hipMemset(g.a, 0, std::max<size_t>(1, (size_t)N * 6) * sizeof(double)));
  HIP_TRY(hipMemset(g.b, 0, std::max<size_t>(1, (size_t)d.M * 3) * sizeof(double)));
  h->gd_ready = true;
  return 0;
}

int ba_gd_begin(ba_handle *h, const ba_options *opt) {
  if (!h || !opt) return fail("ba_gd_begin: bad argument");
  if (!h->finalized && ba_finalize(h)) return -1;
  if (use_device(h)) return -1;
  if (gd_prepare(h, "ba_gd_begin")) return -1;
  if (h->plan.n_obs_global < 1) return fail("ba_gd_begin: num_observations < 1");  // reference :1269
  join_side(h);
  int done_after = 0;
  if (ba::lm_prepare_ctrl(h, opt, &done_after)) return -1;  // (lambda stays initial_lambda: the rows' damping term)
  h->lm_begun = false;
  // previous_cost = EvaluateCurrentCost() (reference :1158) and the first gradient
  ba::launch_gd_pass(h->d, h->gd, h->stream);
  ba::launch_gd_control(h->d, h->gd, 0, h->stream);
  if (done_after) {
    if (pull_ctrl(h)) return -1;
    h->hc.done = 1;
    if (push_ctrl(h)) return -1;
  }
  HIP_TRY(hipGetLastError());
  h->gd_begun = true;
  return 0;
}

int ba_gd_iterate(ba_handle *h, int n) {
  if (!h) return fail("ba_gd_iterate: null handle");
  if (!h->gd_begun)
    return fail(h->lm_begun ? "ba_gd_iterate: the handle is in an LM loop (ba_lm_begin); call ba_gd_begin first"
                            : "ba_gd_iterate: call ba_gd_begin first");
  if (use_device(h)) return -1;
  h->gathered_valid = false;
  for (int k = 0; k < n; ++k) {
    ba::launch_gd_update(h->d, h->gd, h->stream);
    ba::launch_gd_pass(h->d, h->gd, h->stream);
    ba::launch_gd_control(h->d, h->gd, 1, h->stream);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int ba_gd_sync(ba_handle *h, ba_iter_info *out, int cap, int *n_iter, int *converged) {
  if (!h) return fail("ba_gd_sync: null handle");
  if (!h->gd_begun) return fail("ba_gd_sync: call ba_gd_begin first");
  if (use_device(h)) return -1;
  if (pull_ctrl(h)) return -1;
  const int n = h->hc.iter;
  if (n_iter) *n_iter = n;
  if (converged) *converged = h->hc.converged;
  if (out && cap > 0 && n > 0) {
    const int m = std::min(std::min(n, cap), h->d.log_cap);
    HIP_TRY(hipMemcpy(out, h->d.log, (size_t)m * sizeof(ba_iter_info), hipMemcpyDeviceToHost));
  }
  return h->hc.done ? 1 : 0;
}

int ba_solve_gd(ba_handle *h, const ba_options *opt, ba_iter_info *out, int cap, int *n_iter, int *converged) {
  if (ba_gd_begin(h, opt)) return -1;
  int done = opt->max_num_iterations <= 0;
  int issued = 0;
  while (!done) {
    const int batch = std::min(8, opt->max_num_iterations - issued);
    if (batch <= 0) break;
    if (ba_gd_iterate(h, batch)) return -1;
    issued += batch;
    const int rc = ba_gd_sync(h, nullptr, 0, nullptr, nullptr);
    if (rc < 0) return -1;
    done = rc;
  }
  const int rc = ba_gd_sync(h, out, cap, n_iter, converged);
  return rc < 0 ? -1 : 0;
}

int ba_gd_get_gradient(ba_handle *h, double *a6, double *b3) {
  if (!h || !h->finalized) return fail("ba_gd_get_gradient: not finalized");
  if (!h->gd_ready) return fail("ba_gd_get_gradient: call ba_gd_begin first");
  if (use_device(h)) return -1;
  const ba::Plan &pl = h->plan;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (a6 && pl.N > 0) HIP_TRY(hipMemcpy(a6, h->gd.a, (size_t)pl.N * 6 * sizeof(double), hipMemcpyDeviceToHost));
  if (b3) {
    std::vector<double> b;
    if (download(b, h->gd.b, (size_t)pl.M * 3, h->stream)) return -1;
    for (int i = 0; i < pl.M; ++i)
      std::memcpy(b3 + (size_t)pl.iopt_of_user[pl.pt_user_of_int[i]] * 3, &b[(size_t)i * 3], 3 * sizeof(double));
  }
  return 0;
}

// ---------------------------------------------------------------------------
// stage API
int ba_stage_cost(ba_handle *h, double *cost) {
  if (!h || !h->finalized || !cost) return fail("ba_stage_cost: bad argument");
  if (use_device(h)) return -1;
  if (pull_ctrl(h)) return -1;
  h->hc.done = 0;
  if (push_ctrl(h)) return -1;
  join_side(h);
  ba::launch_cost(h->d, 0, 0, h->stream);
  ba::launch_scalars_cost_only(h->d, 0, h->stream);
  if (h->rel.F > 0) {  // + the factors' norms at the accepted poses
    ba::launch_rel_lin(h->d, h->rel, 0, 0, h->stream);
    ba::launch_rel_gather(h->d, h->rel, 0, 2, h->stream);
  }
  if (xchg(h, 1)) return -1;
  HIP_TRY(hipMemcpyAsync(cost, h->d.scal, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

int ba_stage_linearize(ba_handle *h, double lambda, double huber) {
  if (!h || !h->finalized) return fail("ba_stage_linearize: not finalized");
  if (use_device(h)) return -1;
  if (pull_ctrl(h)) return -1;
  h->hc.done = 0;
  h->hc.lambda = lambda;
  h->hc.huber = huber;
  if (push_ctrl(h)) return -1;
  join_side(h);
  enqueue_linearize(h, 0);
  if (h->rel.F > 0) {
    ba::launch_rel_lin(h->d, h->rel, 0, 1, h->stream);
    ba::launch_rel_gather(h->d, h->rel, 0, 1, h->stream);
  }
  ba::launch_damp_invert(h->d, h->stream);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

int ba_stage_schur(ba_handle *h) {
  if (!h || !h->finalized) return fail("ba_stage_schur: not finalized");
  if (use_device(h)) return -1;
  join_side(h);
  ba::launch_schur(h->d, /*direct=*/false, /*with_init=*/true, h->stream);
  if (h->rel.F > 0) ba::launch_rel_offdiag(h->d, h->rel, false, h->stream);
  if (xchg(h, 0)) return -1;
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

int ba_stage_solve_reduced(ba_handle *h) {
  if (!h || !h->finalized) return fail("ba_stage_solve_reduced: not finalized");
  if (use_device(h)) return -1;
  ba::launch_scatter(h->d, h->stream);  // packed (reduced) S||rhs -> dense
  ba::launch_dense_solve(h->d, h->sched, h->ddev, h->stream);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

int ba_stage_backsub_update(ba_handle *h) {
  if (!h || !h->finalized) return fail("ba_stage_backsub_update: not finalized");
  if (use_device(h)) return -1;
  ba::launch_backsub_update(h->d, h->stream);
  if (h->rel.F > 0) ba::launch_rel_lin(h->d, h->rel, 1, 2, h->stream);  // norms at the trial poses, cross term
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  return 0;
}

int ba_stage_scalars(ba_handle *h, double *trial_cost, double *model_change,
                     double *pose_step_sum, double *point_step_sum) {
  if (!h || !h->finalized) return fail("ba_stage_scalars: not finalized");
  if (use_device(h)) return -1;
  ba::launch_cost(h->d, 1, 0, h->stream);
  ba::launch_scalars(h->d, 0, h->stream);
  if (h->rel.F > 0) ba::launch_rel_gather(h->d, h->rel, 1, 6, h->stream);
  if (xchg(h, 1)) return -1;
  double sc[4], pp[2];
  HIP_TRY(hipMemcpyAsync(sc, h->d.scal, sizeof(sc), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(pp, h->d.pose_part, sizeof(pp), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (trial_cost) *trial_cost = sc[0];
  if (model_change) *model_change = -sc[1];
  if (point_step_sum) *point_step_sum = sc[2];
  if (pose_step_sum) *pose_step_sum = pp[1];
  return 0;
}

int ba_stage_commit(ba_handle *h, int accept) {
  if (!h || !h->finalized) return fail("ba_stage_commit: not finalized");
  if (use_device(h)) return -1;
  h->gathered_valid = false;
  if (pull_ctrl(h)) return -1;
  if (accept) h->hc.cur ^= 1;
  if (push_ctrl(h)) return -1;
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

int ba_enable_stage_timing(ba_handle *h, int on) {
  if (!h) return fail("null handle");
  if (use_device(h)) return -1;
  if (on && !h->ev_ok) {
    for (int k = 0; k <= ST_N; ++k) HIP_TRY(hipEventCreate(&h->ev[k]));
    h->ev_ok = true;
  }
  h->timing = on != 0;
  h->kt.on = h->timing;
  return 0;
}

int ba_get_stage_ms(ba_handle *h, double out8[8], int reset) {
  if (!h || !out8) return fail("ba_get_stage_ms: bad argument");
  for (int k = 0; k < 8; ++k) out8[k] = h->stage_ms[k];
  if (reset)
    for (int k = 0; k < 8; ++k) h->stage_ms[k] = 0.0;
  return 0;
}

// ---------------------------------------------------------------------------
// readers
int ba_num_opt_poses(ba_handle *h) { return (h && h->finalized) ? h->plan.N : -1; }
int ba_num_opt_points(ba_handle *h) { return (h && h->finalized) ? h->plan.M : -1; }
// (pairs that a masked covisibility group pads in — no observation, W = 0 — are an
//  internal device of the layout: the readers do not show them)
int64_t ba_num_pairs(ba_handle *h) { return (h && h->finalized) ? h->plan.P - h->plan.n_pair_pad : -1; }
int64_t ba_num_schur_blocks(ba_handle *h) { return (h && h->finalized) ? h->plan.B : -1; }
int64_t ba_num_schur_triples(ba_handle *h) { return (h && h->finalized) ? h->plan.T : -1; }

int ba_get_poses(ba_handle *h, double *T_jw12) {
  if (!h || !h->finalized || !T_jw12) return fail("ba_get_poses: bad argument");
  if (use_device(h) || pull_ctrl(h)) return -1;
  std::vector<double> buf;
  if (download(buf, h->d.poses[h->hc.cur], (size_t)h->plan.n_pose * 12, h->stream)) return -1;
  for (int p = 0; p < h->plan.n_pose; ++p)
    std::memcpy(T_jw12 + (size_t)h->plan.pose_user_of_int[p] * 12, &buf[(size_t)p * 12],
                12 * sizeof(double));
  return 0;
}

// rows of `src` (internal point order) to user order in `dst`
__global__ void k_points_to_user(const double *__restrict__ src, const int32_t *__restrict__ user_of_int, int n,
                                 double *__restrict__ dst) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n) return;
  const size_t u = (size_t)user_of_int[q] * 3;
  dst[u + 0] = src[(size_t)q * 3 + 0];
  dst[u + 1] = src[(size_t)q * 3 + 1];
  dst[u + 2] = src[(size_t)q * 3 + 2];
}

int ba_gather_points(ba_handle *h) {
  if (!h || !h->finalized) return fail("ba_gather_points: not finalized");
  if (use_device(h)) return -1;
  h->gathered_valid = false;
  if (!h->ar_fn || h->world <= 1) return 0;  // one shard owns every point: nothing to gather
  const ba::Plan &pl = h->plan;
  const size_t n3 = (size_t)pl.n_pt_global * 3;
  if (!h->gbuf && h->dalloc(Mem::Resident, &h->gbuf, n3)) return -1;
  if (!h->pt_user_dev && h->upload(Mem::Resident, &h->pt_user_dev, pl.pt_user_of_int)) return -1;
  if (pull_ctrl(h)) return -1;  // `cur` (synchronises the stream)
  join_side(h);
  HIP_TRY(hipMemsetAsync(h->gbuf, 0, n3 * sizeof(double), h->stream));
  if (pl.n_pt > 0)
    hipLaunchKernelGGL(k_points_to_user, dim3((pl.n_pt + 255) / 256), dim3(256), 0, h->stream,
                       (const double *)h->d.pts[h->hc.cur], (const int32_t *)h->pt_user_dev, pl.n_pt, h->gbuf);
  if (h->ar_fn(h->ar_user, 2, (void *)h->gbuf, (int64_t)n3, (void *)h->stream) != 0)
    return fail("ba_gather_points: all-reduce hook returned an error");
  if (download(h->gathered, h->gbuf, n3, h->stream)) return -1;
  HIP_TRY(hipGetLastError());
  h->gathered_valid = true;
  return 0;
}

int ba_get_points(ba_handle *h, double *X3, uint8_t *owned_mask) {
  if (!h || !h->finalized || !X3) return fail("ba_get_points: bad argument");
  if (h->gathered_valid) {  // after ba_gather_points: every point of the full problem
    std::memcpy(X3, h->gathered.data(), h->gathered.size() * sizeof(double));
    if (owned_mask) std::memset(owned_mask, 1, (size_t)h->plan.n_pt_global);
    return 0;
  }
  if (use_device(h) || pull_ctrl(h)) return -1;
  std::vector<double> buf;
  if (download(buf, h->d.pts[h->hc.cur], (size_t)h->plan.n_pt * 3, h->stream)) return -1;
  if (owned_mask) std::memset(owned_mask, 0, (size_t)h->plan.n_pt_global);
  for (int q = 0; q < h->plan.n_pt; ++q) {
    const int u = h->plan.pt_user_of_int[q];
    std::memcpy(X3 + (size_t)u * 3, &buf[(size_t)q * 3], 3 * sizeof(double));
    if (owned_mask) owned_mask[u] = 1;
  }
  return 0;
}

int ba_get_A(ba_handle *h, double *A36, double *a6) {
  if (!h || !h->finalized) return fail("ba_get_A: not finalized");
  if (use_device(h)) return -1;
  join_side(h);
  if (pull_ctrl(h)) return -1;  // synchronises the stream
  const int lb = h->hc.lcur;
  if (A36) {
    HIP_TRY(hipMemcpy(A36, h->d.A[lb], (size_t)h->plan.N * 36 * sizeof(double), hipMemcpyDeviceToHost));
    // the device keeps A_j undamped and scales the diagonal where it reads it
    // (reference :833-844): the same scaling here
    const double lp1 = 1.0 + h->hc.lambda;
    for (int j = 0; j < h->plan.N; ++j)
      for (int r = 0; r < 6; ++r) A36[(size_t)j * 36 + r * 7] *= lp1;
  }
  if (a6) HIP_TRY(hipMemcpy(a6, h->d.a[lb], (size_t)h->plan.N * 6 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

static void expand_sym3(const double *s6, double *f9) {
  f9[0] = s6[0]; f9[1] = s6[1]; f9[2] = s6[2];
  f9[3] = s6[1]; f9[4] = s6[3]; f9[5] = s6[4];
  f9[6] = s6[2]; f9[7] = s6[4]; f9[8] = s6[5];
}

static int get_sym_vec(ba_handle *h, const double *dS6, const double *dV3,
                       double *out9, double *out3) {
  const ba::Plan &pl = h->plan;
  std::vector<double> s6, v3;
  if (download(s6, dS6, (size_t)pl.M * 6, h->stream)) return -1;
  if (download(v3, dV3, (size_t)pl.M * 3, h->stream)) return -1;
  for (int i = 0; i < pl.M; ++i) {
    const int g = pl.iopt_of_user[pl.pt_user_of_int[i]];
    if (out9) expand_sym3(&s6[(size_t)i * 6], out9 + (size_t)g * 9);
    if (out3) std::memcpy(out3 + (size_t)g * 3, &v3[(size_t)i * 3], 3 * sizeof(double));
  }
  return 0;
}

int ba_get_C(ba_handle *h, double *C9, double *b3) {
  if (!h || !h->finalized) return fail("ba_get_C: not finalized");
  if (use_device(h)) return -1;
  join_side(h);
  if (pull_ctrl(h)) return -1;
  ba::launch_damp_invert_export(h->d, h->stream);  // damped C_i of the current block buffer and lambda
  return get_sym_vec(h, h->d.Cd, h->d.b[h->hc.lcur], C9, b3);
}

int ba_get_Cinv(ba_handle *h, double *Cinv9, double *Cinvb3) {
  if (!h || !h->finalized) return fail("ba_get_Cinv: not finalized");
  if (use_device(h)) return -1;
  // Cinv_i b_i is not stored on the device (k_backsub_update forms it): same expression here
  const ba::Plan &pl = h->plan;
  std::vector<double> s6, b3;
  join_side(h);
  if (pull_ctrl(h)) return -1;
  ba::launch_damp_invert_export(h->d, h->stream);  // (the LM loop keeps Cinv in registers where it can)
  if (download(s6, h->d.Cinv, (size_t)pl.M * 6, h->stream)) return -1;
  if (download(b3, h->d.b[h->hc.lcur], (size_t)pl.M * 3, h->stream)) return -1;
  for (int i = 0; i < pl.M; ++i) {
    const int g = pl.iopt_of_user[pl.pt_user_of_int[i]];
    const double *ci = &s6[(size_t)i * 6], *b = &b3[(size_t)i * 3];
    if (Cinv9) expand_sym3(ci, Cinv9 + (size_t)g * 9);
    if (Cinvb3) {
      double *o = Cinvb3 + (size_t)g * 3;
      o[0] = ci[0] * b[0] + ci[1] * b[1] + ci[2] * b[2];
      o[1] = ci[1] * b[0] + ci[3] * b[1] + ci[4] * b[2];
      o[2] = ci[2] * b[0] + ci[4] * b[1] + ci[5] * b[2];
    }
  }
  return 0;
}

void ba_expand_pair_slim(const double *rec8, const double *T12, const double *X3, double *k12) {
  ba::pair_from_G(rec8, rec8[6], T12, X3[0], X3[1], X3[2], k12, k12 + 9);
}

void ba_pair_G_from_obs(const double *cam16, const double *T12, const double *X3, const double *uv2, double huber,
                        double *rec8) {
  ba::pair_G_from_obs(cam16, T12, X3[0], X3[1], X3[2], uv2[0], uv2[1], huber, rec8, rec8[6]);
  rec8[7] = 0.0;
}

int ba_get_pair_form(ba_handle *h) {
  if (!h || !h->finalized) return fail("ba_get_pair_form: not finalized");
  return h->d.pair_obs ? 2 : (h->d.pair_slim ? 1 : 0);
}

int ba_get_slim_records(ba_handle *h, int32_t *pose, int32_t *lm, int32_t *cam, double *uv2, double *rec8) {
  if (!h || !h->finalized) return fail("ba_get_slim_records: not finalized");
  if (use_device(h)) return -1;
  const ba::Plan &pl = h->plan;
  const int64_t n = h->d.P_slim;
  if (pull_ctrl(h)) return -1;  // synchronises the stream
  if (rec8 && n > 0) {
    if (h->d.pair_obs) {
      ba::launch_pair_records(h->d, h->stream);
      HIP_TRY(hipStreamSynchronize(h->stream));
    }
    HIP_TRY(hipMemcpy(rec8, h->d.W[h->hc.lcur], (size_t)n * ba::kWSlim * sizeof(double), hipMemcpyDeviceToHost));
  }
  for (int64_t p = 0; p < n; ++p) {
    if (pose) pose[p] = pl.pose_user_of_int[pl.pair_pose[p]];
    if (lm) lm[p] = pl.pt_user_of_int[pl.pair_lm[p]];
  }
  if (cam || uv2) {
    // the last writer of every grouped pair, from the patterns of the group pieces
    for (const auto &g : pl.lin_desc)
      for (int oo = 0; oo < g.no; ++oo) {
        const int y = pl.grp_pat[2 * ((size_t)g.pat0 + oo) + 1];
        if (!((y >> 30) & 1)) continue;
        const int jj = (y >> 16) & 0xff;
        for (int il = 0; il < g.nl; ++il) {
          const int64_t p = g.p0 + (int64_t)il * g.d + jj, o = g.o0 + (int64_t)il * g.no + oo;
          if (p >= n) continue;
          if (cam) cam[p] = y & 0xffff;
          if (uv2) {
            uv2[2 * p] = pl.obs_uv[2 * o];
            uv2[2 * p + 1] = pl.obs_uv[2 * o + 1];
          }
        }
      }
  }
  return 0;
}

int ba_get_pairs(ba_handle *h, int32_t *pair_i, int32_t *pair_j, double *W18) {
  if (!h || !h->finalized) return fail("ba_get_pairs: not finalized");
  if (use_device(h)) return -1;
  const ba::Plan &pl = h->plan;
  auto padded = [&](int64_t p) { return !pl.pair_pad.empty() && pl.pair_pad[p]; };
  {
    int64_t o = 0;
    for (int64_t p = 0; p < pl.P; ++p) {
      if (padded(p)) continue;
      if (pair_i) pair_i[o] = pl.iopt_of_user[pl.pt_user_of_int[pl.pair_lm[p]]];
      if (pair_j) pair_j[o] = pl.pair_pose[p];
      ++o;
    }
  }
  if (W18) {
    if (pull_ctrl(h)) return -1;  // synchronises the stream
    // the device keeps B_ji compact ({K, X_ij}, ba_device.h kWStride): expand
    std::vector<double> w12((size_t)pl.P * ba::kWStride);
    if (h->d.pair_obs) {  // the iteration keeps no record of the grouped pairs: fill the slim ones
      ba::launch_pair_records(h->d, h->stream);
      HIP_TRY(hipStreamSynchronize(h->stream));
    }
    if (pl.P > 0)
      HIP_TRY(hipMemcpy(w12.data(), h->d.W[h->hc.lcur], w12.size() * sizeof(double), hipMemcpyDeviceToHost));
    // the slim pairs ({G, w}, ba_device.h kWSlim) first become {K, X_ij}, from the poses and
    // points the blocks were linearised at: the accepted ones (cur flips together with lcur)
    const int64_t P_slim = h->d.P_slim;
    std::vector<double> Th, Xh;
    if (P_slim > 0) {
      Th.resize((size_t)pl.n_pose * 12);
      Xh.resize((size_t)pl.M * 3);
      HIP_TRY(hipMemcpy(Th.data(), h->d.poses[h->hc.cur], Th.size() * sizeof(double), hipMemcpyDeviceToHost));
      HIP_TRY(hipMemcpy(Xh.data(), h->d.pts[h->hc.cur], Xh.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    int64_t o = 0;
    for (int64_t p = 0; p < pl.P; ++p) {
      if (padded(p)) continue;
      double k12[12];
      const double *k = &w12[(size_t)p * ba::kWStride];
      if (p < P_slim) {
        ba_expand_pair_slim(&w12[(size_t)p * ba::kWSlim], &Th[(size_t)pl.pair_pose[p] * 12], &Xh[(size_t)pl.pair_lm[p] * 3], k12);
        k = k12;
      }
      double *W = W18 + (size_t)o * 18;
      for (int e = 0; e < 9; ++e) W[e] = k[e];
      for (int c = 0; c < 3; ++c) {
        W[9 + c] = k[10] * k[6 + c] - k[11] * k[3 + c];
        W[12 + c] = k[11] * k[c] - k[9] * k[6 + c];
        W[15 + c] = k[9] * k[3 + c] - k[10] * k[c];
      }
      ++o;
    }
  }
  return 0;
}

int ba_get_S(ba_handle *h, double *S, double *rhs) {
  if (!h || !h->finalized) return fail("ba_get_S: not finalized");
  if (use_device(h)) return -1;
  const ba::DevProblem &d = h->d;
  const int n6 = 6 * h->plan.N;
  std::vector<double> L;
  ba::launch_scatter(d, h->stream);  // from the packed exchange buffer
  if (download(L, d.L, (size_t)d.npad * d.ld, h->stream)) return -1;
  auto colof = [&](int e) { return h->pose_col_h[e / 6] + e % 6; };
  for (int c = 0; c < n6; ++c) {
    for (int r = c; r < n6; ++r) {
      int rr = colof(r), cc = colof(c);
      if (rr < cc) std::swap(rr, cc);
      const double v = L[(size_t)cc * d.ld + rr];
      if (S) {
        S[(size_t)r * n6 + c] = v;
        S[(size_t)c * n6 + r] = v;
      }
    }
    if (rhs) rhs[c] = L[(size_t)colof(c) * d.ld + d.npad];
  }
  return 0;
}

int ba_get_xy(ba_handle *h, double *x6, double *y3) {
  if (!h || !h->finalized) return fail("ba_get_xy: not finalized");
  if (use_device(h)) return -1;
  const ba::Plan &pl = h->plan;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (x6 && pl.N > 0)
    HIP_TRY(hipMemcpy(x6, h->d.x, (size_t)pl.N * 6 * sizeof(double), hipMemcpyDeviceToHost));
  if (y3) {
    std::vector<double> y;
    if (download(y, h->d.y, (size_t)pl.M * 3, h->stream)) return -1;
    for (int i = 0; i < pl.M; ++i) {
      const int g = pl.iopt_of_user[pl.pt_user_of_int[i]];
      std::memcpy(y3 + (size_t)g * 3, &y[(size_t)i * 3], 3 * sizeof(double));
    }
  }
  return 0;
}

// ---------------------------------------------------------------------------
int ba_kernel_count(void) { return ba::K_COUNT; }

const char *ba_kernel_name(int id) {
  static const char *names[ba::K_COUNT] = {
      "k_cost", "k_lin_landmarks", "k_lin_poses", "k_pose_finalize", "k_dense_init",
      "k_schur_lds", "k_schur_partial", "k_schur_final", "k_scatter",
      "k_chol_diag", "k_chol_trsm", "k_chol_update", "k_chol_back", "k_chol_diag_trsm", "k_chol_tail", "k_backsub_update",
      "k_pose_update", "k_scalars", "k_control", "k_damp_invert", "k_schur_grp", "k_lin_grp",
      "k_rel_lin", "k_rel_gather", "k_rel_offdiag",
      "k_s3_lin", "k_s3_assemble", "k_s3_trial", "k_s3_lin_robust", "k_s3_assemble_robust",
      "k_pg_lin_robust", "k_pg_assemble_robust",
      "k_pg_lin", "k_pg_assemble", "k_pg_trial", "k_pg_control"};
  return (id >= 0 && id < ba::K_COUNT) ? names[id] : "";
}

int ba_get_kernel_ms(ba_handle *h, double *ms_out, int64_t *calls_out, int reset) {
  if (!h || !ms_out || !calls_out) return fail("ba_get_kernel_ms: bad argument");
  for (int k = 0; k < ba::K_COUNT; ++k) {
    ms_out[k] = h->kt.ms[k];
    calls_out[k] = h->kt.calls[k];
  }
  if (reset) h->kt.reset();
  return 0;
}

int ba_get_dense_info(ba_handle *h, double out4[4]) {
  if (!h || !h->finalized || !out4) return fail("ba_get_dense_info: bad argument");
  out4[0] = h->sched.fill;
  out4[1] = h->sched.flops;
  out4[2] = (double)h->sched.nlev;
  out4[3] = (double)h->d.npad;
  return 0;
}

int ba_get_schur_info(ba_handle *h, int64_t out8[8]) {
  if (!h || !h->finalized || !out8) return fail("ba_get_schur_info: bad argument");
  const ba::Plan &pl = h->plan;
  int64_t pairs = 0, triples = 0, mfma = 0;
  for (const auto *list : {&pl.grp32, &pl.grp64, &pl.grp128})
    for (const auto &g : *list) {
      pairs += (int64_t)g.nl * g.d;
      triples += (int64_t)g.nl * g.d * (g.d + 1) / 2;
      // v_mfma_f64_16x16x4 instructions of k_schur_grp: chunks of nlw landmarks,
      // ceil(3 nlc / 4) k steps each, NT (NT + 1) / 2 tiles per step
      const int nt = list == &pl.grp32 ? 2 : (list == &pl.grp64 ? 4 : 8), krw = nt == 2 ? 36 : (nt == 4 ? 20 : 8);
      const int nlw = std::min(64 / g.d, krw / 3);
      for (int c0 = 0; c0 < g.nl; c0 += nlw)
        mfma += (int64_t)((3 * std::min(nlw, g.nl - c0) + 3) / 4) * (nt * (nt + 1) / 2);
    }
  out8[0] = (int64_t)pl.grp32.size();
  out8[1] = (int64_t)(pl.grp64.size() + pl.grp128.size());  // (64- and 128-wide images)
  out8[2] = pl.M_grp;
  out8[3] = (int64_t)pl.sup_desc.size();
  out8[4] = pairs;
  out8[5] = triples;
  out8[6] = mfma;
  out8[7] = (int64_t)pl.tri_p.size();
  return 0;
}

int ba_get_lin_info(ba_handle *h, int64_t out4[4]) {
  if (!h || !h->finalized || !out4) return fail("ba_get_lin_info: bad argument");
  const ba::Plan &pl = h->plan;
  int64_t obs = 0;
  for (const auto &g : pl.lin_desc) obs += (int64_t)g.nl * g.no;
  out4[0] = (int64_t)pl.lin_desc.size();
  out4[1] = obs;
  out4[2] = (int64_t)pl.bchunk_lm.size() - 1 - (pl.lin_groups ? pl.n_bchunk_grp : 0);
  out4[3] = pl.n_pobs;
  return 0;
}

int ba_get_pair_record_info(ba_handle *h, int64_t out2[2]) {
  if (!h || !h->finalized || !out2) return fail("ba_get_pair_record_info: bad argument");
  out2[0] = h->d.P_slim;
  out2[1] = h->plan.P;
  return 0;
}

int ba_get_mask_info(ba_handle *h, int64_t out4[4]) {
  if (!h || !h->finalized || !out4) return fail("ba_get_mask_info: bad argument");
  const ba::Plan &pl = h->plan;
  int64_t lm = 0;
  for (const auto &g : pl.grp_range) lm += g.masked ? g.nl : 0;
  out4[0] = (int64_t)pl.lin_desc.size() - pl.n_lin_plain;
  out4[1] = lm;
  out4[2] = pl.n_obs - (pl.n_obs_global > 0 && h->world == 1 ? pl.n_obs_global : pl.n_obs);
  {  // (sharded: count the padded slots themselves)
    int64_t pad = 0;
    for (int64_t s2 = 0; s2 < pl.n_obs; ++s2) pad += !(pl.obs_uv[2 * s2] == pl.obs_uv[2 * s2]);
    out4[2] = pad;
  }
  out4[3] = pl.n_pair_pad;
  return 0;
}

int ba_get_dropped_pivots(ba_handle *h, int64_t *count, int reset) {
  if (!h || !h->finalized || !count) return fail("ba_get_dropped_pivots: bad argument");
  if (use_device(h)) return -1;
  int v = 0;
  HIP_TRY(hipMemcpyAsync(&v, h->ddev.bad_pivots, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (reset) HIP_TRY(hipMemsetAsync(h->ddev.bad_pivots, 0, sizeof(int), h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  *count = v % ba::kFlowTimeout;  // (the upper bits count timed-out hand-offs: ba_lm_sync reports those)
  return 0;
}

int ba_dense_spd_solve(ba_handle *h, int n, const double *A, const double *b,
                       double *x, double *ms) {
  if (!h || n <= 0 || !A || !b || !x) return fail("ba_dense_spd_solve: bad argument");
  if (use_device(h)) return -1;
  // a dense matrix has one tile per level either way: fewer, larger tiles (BA_DENSE_NB=32 for a
  // sparse system, or to test the 32-column kernels alone)
  const int nb = h->knobs.dense.nb == 32 ? 32 : 64;
  const int ncb = (n + nb - 1) / nb;
  const int npad = ncb * nb;
  const int ld = npad + nb;
  // tile pattern of A -> level schedule -> symmetric tile permutation
  std::vector<uint8_t> adj((size_t)ncb * ncb, 0);
  for (int I = 0; I < ncb; ++I)
    for (int J = 0; J < I; ++J) {
      bool any = false;
      for (int r = I * nb; r < std::min(n, (I + 1) * nb) && !any; ++r)
        for (int c = J * nb; c < (J + 1) * nb && !any; ++c) any = A[(size_t)r * n + c] != 0.0;
      adj[(size_t)I * ncb + J] = adj[(size_t)J * ncb + I] = any;
    }
  ba::DenseSchedule sc;
  ba::build_dense_schedule(ncb, adj, h->knobs.dense.natural, nb, sc, h->knobs.dense.order);
  std::vector<int> colmap(npad), col_x(npad, -1);  // original column -> dense column
  for (int c = 0; c < npad; ++c) colmap[c] = sc.pos_of_tile[c / nb] * nb + c % nb;
  std::vector<double> L((size_t)npad * ld, 0.0);
  for (int c = 0; c < npad; ++c) {
    if (c < n) {
      col_x[colmap[c]] = c;
      for (int r = c; r < n; ++r) {
        int rr = colmap[r], cc = colmap[c];
        if (rr < cc) std::swap(rr, cc);
        L[(size_t)cc * ld + rr] = A[(size_t)r * n + c];
      }
      L[(size_t)colmap[c] * ld + npad] = b[c];
    } else {
      L[(size_t)colmap[c] * ld + colmap[c]] = 1.0;
    }
  }
  // everything below is allocated on the handle and freed again on every return, so that
  // repeated calls do not grow the handle's memory
  ba::ScratchAllocs scratch(h);
  ba::DenseDev dd;
  double *dL = nullptr, *dD = nullptr, *dx = nullptr;
  if (upload_dense_schedule(h, sc, col_x, dd) || h->upload(Mem::Resident, &dL, L) ||
      h->dalloc(Mem::Resident, &dD, (size_t)ncb * ba::dense_ws_per_block(nb)) || h->dalloc(Mem::Resident, &dx, (size_t)npad))
    return -1;
  hipEvent_t e0, e1;
  HIP_TRY(hipEventCreate(&e0));
  HIP_TRY(hipEventCreate(&e1));
  HIP_TRY(hipEventRecord(e0, h->stream));
  ba::dense_factor_solve(dL, npad, ld, dD, dx, nullptr, sc, dd, dd.plan[dd.flow_ok], h->stream);
  HIP_TRY(hipEventRecord(e1, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  float t = 0.f;
  (void)hipEventElapsedTime(&t, e0, e1);
  if (ms) *ms = t;
  HIP_TRY(hipMemcpy(x, dx, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
  int bad_h = 0;
  HIP_TRY(hipMemcpy(&bad_h, dd.bad_pivots, sizeof(int), hipMemcpyDeviceToHost));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  HIP_TRY(hipGetLastError());
  if (bad_h >= ba::kFlowTimeout) return fail("ba_dense_spd_solve: a dataflow hand-off timed out");
  return 0;
}

// ---------------------------------------------------------------------------
// covariance blocks (kernels: ba_cov.hip)
int ba_covariance_check(int finalized, int sharded, int streamed, int n_pose, const uint8_t *pose_fixed,
                        int n_pt, const uint8_t *pt_fixed, int n_pose_sel, const int32_t *pose_sel,
                        const double *cov_pose36, int n_pt_sel, const int32_t *pt_sel,
                        const double *cov_pt9) {
  if (!finalized) return fail("ba_covariance: the handle is not finalized");
  if (sharded) return fail("ba_covariance: sharded handles (ba_set_shard world > 1, or an all-reduce hook) are not supported");
  if (streamed) return fail("ba_covariance: streamed handles are not supported");
  if (n_pose_sel < 0 || n_pt_sel < 0) return fail("ba_covariance: negative selection size");
  if (n_pose_sel > 0 && !pose_sel) return fail("ba_covariance: pose_sel is NULL for a non-empty selection");
  if (n_pt_sel > 0 && !pt_sel) return fail("ba_covariance: pt_sel is NULL for a non-empty selection");
  if (n_pose_sel > 0 && !cov_pose36) return fail("ba_covariance: cov_pose36 is NULL for a non-empty pose selection");
  if (n_pt_sel > 0 && !cov_pt9) return fail("ba_covariance: cov_pt9 is NULL for a non-empty point selection");
  for (int s = 0; s < n_pose_sel; ++s) {
    const int u = pose_sel[s];
    if (u < 0 || u >= n_pose)
      return fail("ba_covariance: pose_sel[" + std::to_string(s) + "] = " + std::to_string(u) + " is out of range");
    if (pose_fixed && pose_fixed[u])
      return fail("ba_covariance: pose_sel[" + std::to_string(s) + "] = " + std::to_string(u) + " is a fixed pose");
  }
  for (int s = 0; s < n_pt_sel; ++s) {
    const int u = pt_sel[s];
    if (u < 0 || u >= n_pt)
      return fail("ba_covariance: pt_sel[" + std::to_string(s) + "] = " + std::to_string(u) + " is out of range");
    if (pt_fixed && pt_fixed[u])
      return fail("ba_covariance: pt_sel[" + std::to_string(s) + "] = " + std::to_string(u) + " is a fixed point");
  }
  return 0;
}

using ba::cov_batch_cols;  // ba_handle.h: shared with ba_pgraph_covariance

int ba_covariance_info(ba_handle *h, int64_t out4[4]) {
  if (!h || !h->finalized || !out4) return fail("ba_covariance_info: bad argument");
  const int bw = cov_batch_cols(h->d.npad, h->knobs.run);
  out4[0] = bw;
  out4[1] = ba::kCovGroupCols;
  out4[2] = (int64_t)h->d.npad * bw * (int64_t)sizeof(double);
  out4[3] = h->cov_batches;
  return 0;
}

int ba_covariance(ba_handle *h, double huber, int n_pose_sel, const int32_t *pose_sel, double *cov_pose36,
                  int n_pt_sel, const int32_t *pt_sel, double *cov_pt9, int64_t *dropped_pivots) {
  if (!h) return fail("ba_covariance: null handle");
  if (ba_covariance_check(h->finalized, h->world > 1 || h->ar_fn != nullptr,
                          h->arena != nullptr || h->dense_owner != nullptr, h->n_pose,
                          h->pose_fixed.data(), h->n_pt, h->pt_fixed.data(), n_pose_sel, pose_sel,
                          cov_pose36, n_pt_sel, pt_sel, cov_pt9))
    return -1;
  if (use_device(h)) return -1;
  const ba::Plan &pl = h->plan;
  const ba::DevProblem &d = h->d;
  const ba::DenseSchedule &sc = h->sched;
  const int nb = d.nb, ncb = sc.ncb;
  // ---- distinct items, ordered by the tile of their first non-zero row, in groups of one wave
  struct Item {
    int t0, key, idx;
  };
  auto distinct = [](std::vector<Item> &v) {
    std::sort(v.begin(), v.end(), [](const Item &a, const Item &b) {
      return a.t0 != b.t0 ? a.t0 < b.t0 : a.key != b.key ? a.key < b.key : a.idx < b.idx;
    });
    v.erase(std::unique(v.begin(), v.end(), [](const Item &a, const Item &b) { return a.idx == b.idx; }), v.end());
  };
  std::vector<Item> poses, pts;
  for (int s = 0; s < n_pose_sel; ++s) {
    const int j = pl.jopt_of_user[pose_sel[s]];
    poses.push_back({h->pose_col_h[j] / nb, h->pose_col_h[j], j});
  }
  for (int s = 0; s < n_pt_sel; ++s) {
    const int i = pl.pt_int_of_user[pt_sel[s]];
    if (i < 0 || i >= pl.M) return fail("ba_covariance: pt_sel[" + std::to_string(s) + "] is not an optimisable point of this handle");
    int t0 = ncb;  // (no pairs: zero right-hand side, nothing to sweep)
    for (int64_t p = pl.lm_pair_ptr[i]; p < pl.lm_pair_ptr[i + 1]; ++p)
      t0 = std::min(t0, h->pose_col_h[pl.pair_pose[p]] / nb);
    pts.push_back({t0, i, i});
  }
  distinct(poses);
  distinct(pts);
  std::vector<int> slot_pose(pl.N, -1), slot_pt(pl.M, -1);
  std::vector<ba::CovGroup> groups;
  auto make_groups = [&](const std::vector<Item> &v, int kind, int per, std::vector<int> &slot) {
    for (size_t k = 0; k < v.size(); k += per) {
      ba::CovGroup g{};
      g.kind = kind;
      g.n = (int)std::min<size_t>(per, v.size() - k);
      g.t0 = v[k].t0;
      for (int a = 0; a < g.n; ++a) {
        g.item[a] = v[k + a].idx;
        g.slot[a] = slot[v[k + a].idx] = (int)(k + a);
      }
      groups.push_back(g);
    }
  };
  make_groups(poses, 0, 2, slot_pose);
  make_groups(pts, 1, 5, slot_pt);
  // per tile position: the positions left of it with a non-zero factor tile
  std::vector<int> trow_ptr((size_t)ncb + 1, 0), trow;
  {
    std::vector<std::vector<int>> by_row((size_t)ncb);
    for (int p = 0; p < ncb; ++p)
      for (int a = sc.row_ptr[p]; a < sc.row_ptr[p + 1]; ++a)
        if (sc.rows[a] < ncb) by_row[sc.rows[a]].push_back(p);
    for (int t = 0; t < ncb; ++t) {
      trow.insert(trow.end(), by_row[t].begin(), by_row[t].end());
      trow_ptr[t + 1] = (int)trow.size();
    }
  }
  // ---- linearise at lambda = 0, Schur complement, scatter, factorise (the stage calls' launches)
  join_side(h);
  if (pull_ctrl(h)) return -1;
  const ba::DevCtrl keep = h->hc;
  h->hc.done = 0;
  h->hc.lambda = 0.0;
  h->hc.huber = huber;
  if (push_ctrl(h)) return -1;
  int bad_keep = 0, bad_now = 0;
  // (the stream is idle: pull_ctrl synchronised it)  the LM loop's count of dropped pivots is set
  // aside, this call's factorisation counts from zero, and the loop's count comes back below
  HIP_TRY(hipMemcpy(&bad_keep, h->ddev.bad_pivots, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemsetAsync(h->ddev.bad_pivots, 0, sizeof(int), h->stream));
  enqueue_linearize(h, 0);
  ba::launch_pair_records(d, h->stream);  // (pair_obs: k_cov_rhs reads slim records, the iteration keeps none)
  if (h->rel.F > 0) {
    ba::launch_rel_lin(d, h->rel, 0, 1, h->stream);
    ba::launch_rel_gather(d, h->rel, 0, 1, h->stream);
  }
  ba::launch_damp_invert_export(d, h->stream);  // Cinv_i as an array, whatever Schur path the plan uses
  ba::launch_schur(d, /*direct=*/false, /*with_init=*/true, h->stream);
  if (h->rel.F > 0) ba::launch_rel_offdiag(d, h->rel, false, h->stream);
  ba::launch_scatter(d, h->stream);
  {
    // k_chol_tail keeps its block's factor in LDS (only x leaves): here no level goes to it, so
    // that the whole factor is left in the image.  Same arithmetic.
    const ba::DenseDev &dd = h->ddev;
    ba::dense_factor_solve(d.L, d.npad, d.ld, d.Ldiag, d.x, &d.ctrl->done, sc, dd,
                           ba::dense_launch_plan_no_tail(sc, h->knobs.dense, dd.flow_ok, dd.plan[1], h->knobs.cone.want), h->stream);
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipMemcpy(&bad_now, h->ddev.bad_pivots, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(h->ddev.bad_pivots, &bad_keep, sizeof(int), hipMemcpyHostToDevice));
  h->hc = keep;  // the controller as it was: lambda, huber, done, the log position
  if (push_ctrl(h)) return -1;
  // ---- the batches; everything below is freed again on every return
  ba::ScratchAllocs scratch(h);
  const int bw_max = cov_batch_cols(d.npad, h->knobs.run);
  const int gpb = bw_max / ba::kCovGroupCols;  // groups per batch
  const int bw = (int)std::min<size_t>(gpb, std::max<size_t>(1, groups.size())) * ba::kCovGroupCols;
  int *d_trow_ptr = nullptr, *d_trow = nullptr;
  ba::CovGroup *d_groups = nullptr;
  double *Zw = nullptr, *d_pose = nullptr, *d_pt = nullptr;
  if (h->upload(Mem::Resident, &d_trow_ptr, trow_ptr) || h->upload(Mem::Resident, &d_trow, trow) ||
      h->upload(Mem::Resident, &d_groups, groups) ||
      h->dalloc(Mem::Resident, &Zw, (size_t)d.npad * bw) || h->dalloc(Mem::Resident, &d_pose, poses.size() * 36) ||
      h->dalloc(Mem::Resident, &d_pt, pts.size() * 9))
    return -1;
  h->cov_batches = 0;
  for (size_t g0 = 0; g0 < groups.size(); g0 += gpb) {  // fixed batch order
    const int ng = (int)std::min<size_t>(gpb, groups.size() - g0);
    ba::launch_cov_batch(d, keep.lcur, keep.cur, ncb, d_trow_ptr, d_trow, d_groups + g0, ng, Zw, bw, d_pose, d_pt, h->stream);
    ++h->cov_batches;
  }
  std::vector<double> hp, hq;
  if (download(hp, d_pose, poses.size() * 36, h->stream) || download(hq, d_pt, pts.size() * 9, h->stream)) return -1;
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  if (bad_now >= ba::kFlowTimeout) return fail("ba_covariance: a dataflow hand-off of the factorisation timed out");
  for (int s = 0; s < n_pose_sel; ++s)
    std::memcpy(cov_pose36 + (size_t)s * 36, &hp[(size_t)slot_pose[pl.jopt_of_user[pose_sel[s]]] * 36], 36 * sizeof(double));
  for (int s = 0; s < n_pt_sel; ++s)
    std::memcpy(cov_pt9 + (size_t)s * 9, &hq[(size_t)slot_pt[pl.pt_int_of_user[pt_sel[s]]] * 9], 9 * sizeof(double));
  if (dropped_pivots) *dropped_pivots = bad_now;
  return 0;
}

}  // extern "C" (reopened below)

// One call = one H2D copy, one kernel, one D2H copy, all through ONE pinned
// staging buffer that mirrors ONE device buffer (ten small pageable copies
// cost more than the kernel at 10 k points):
//   [X | uv | uv_right | right camera | T | mask | mask_right | barrier words ]  <- H2D
//                                     [ T | mask | mask_right | barrier words | meta | iters | debug poses ]  <- D2H
namespace {
struct PoLayout {
  size_t X, uv, uvr, camr, T, mask, maskr, gsw, h2d_end, meta, iters, dbg, end;
};
PoLayout po_layout(int n, int icap, bool stereo) {
  auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
  PoLayout L;
  size_t o = 0;
  L.X = o;      o = al(o + (size_t)n * 3 * sizeof(float));
  L.uv = o;     o = al(o + (size_t)n * 2 * sizeof(float));
  L.uvr = o;    o = al(o + (stereo ? (size_t)n * 2 * sizeof(float) : 0));
  L.camr = o;   o = al(o + 16 * sizeof(float));
  L.T = o;      o = al(o + 12 * sizeof(float));
  L.mask = o;   o = al(o + (size_t)n);
  L.maskr = o;  o = al(o + (stereo ? (size_t)n : 0));
  L.gsw = o;    o = al(o + sizeof(int) * (size_t)ba::pose_only_sync_ints());
  L.h2d_end = o;
  L.meta = o;   o = al(o + 4 * sizeof(int));
  L.iters = o;  o = al(o + (size_t)icap * sizeof(ba::PoIter));
  L.dbg = o;    o = al(o + (size_t)icap * 12 * sizeof(float));
  L.end = o;
  return L;
}

// grow the pose-only buffer pair to `bytes` (not in `allocs`: freed here and in
// free_device)
int po_reserve(ba_handle *h, size_t bytes) {
  if (bytes <= h->po_cap) return 0;
  if (h->po_dev) (void)hipFree(h->po_dev);
  if (h->po_host) (void)hipHostFree(h->po_host);
  h->po_dev = h->po_host = nullptr;
  h->po_cap = 0;
  HIP_TRY(hipMalloc((void **)&h->po_dev, bytes));
  HIP_TRY(hipHostMalloc((void **)&h->po_host, bytes, hipHostMallocDefault));
  h->po_cap = bytes;
  return 0;
}

// right camera record of the stereo 6-DoF solvers: fx fy cx cy, then
// pose_right_to_left = left_to_right^-1 (reference :226) as R (9, row-major) and t (3)
void po_right_camera(const float *intr_r4, const float *T_lr12, float *camr) {
  for (int k = 0; k < 4; ++k) camr[k] = intr_r4[k];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) camr[4 + r * 3 + c] = T_lr12[c * 3 + r];
  for (int r = 0; r < 3; ++r)
    camr[13 + r] = -(camr[4 + r * 3 + 0] * T_lr12[9] + camr[4 + r * 3 + 1] * T_lr12[10] +
                     camr[4 + r * 3 + 2] * T_lr12[11]);
}

int po_run(ba_handle *h, bool stereo, const float *X3, const float *uv2, const float *uvr2, int n,
           float fx, float fy, float cx, float cy, const float *camr16, float *T12, uint8_t *mask,
           uint8_t *mask_r, const ba_options *opt, ba_po_iter *iters, int cap, int *n_iter,
           int *converged, float *debug_T12, const ba::Po3Params *p3 = nullptr) {
  // p3 != nullptr: the planar 3-DoF kernel (T12 = world_to_current, camr unused)
  if (use_device(h)) return -1;
  static_assert(sizeof(ba::PoIter) == sizeof(ba_po_iter), "po iter layout");
  const int max_it = opt->max_num_iterations;
  const int icap = std::max(1, std::max(cap, max_it));
  const PoLayout L = po_layout(n, icap, stereo);
  if (po_reserve(h, L.end)) return -1;
  if (!h->po_part && h->dalloc(Mem::Resident, &h->po_part, (size_t)ba::pose_only_partial_floats())) return -1;
  uint8_t *hb = h->po_host, *db = h->po_dev;
  std::memcpy(hb + L.X, X3, (size_t)n * 3 * sizeof(float));
  std::memcpy(hb + L.uv, uv2, (size_t)n * 2 * sizeof(float));
  if (stereo) {
    std::memcpy(hb + L.uvr, uvr2, (size_t)n * 2 * sizeof(float));
    if (camr16) std::memcpy(hb + L.camr, camr16, 16 * sizeof(float));
    std::memcpy(hb + L.maskr, mask_r, (size_t)n);
  }
  std::memcpy(hb + L.T, T12, 12 * sizeof(float));
  std::memcpy(hb + L.mask, mask, (size_t)n);
  std::memset(hb + L.gsw, 0, sizeof(int) * (size_t)ba::pose_only_sync_ints());
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpyAsync(db, hb, L.h2d_end, hipMemcpyHostToDevice, s));
  float *dT = (float *)(db + L.T), *ddbg = debug_T12 ? (float *)(db + L.dbg) : nullptr;
  int rc;
  if (p3)
    rc = ba::pose_only_planar3_device(
        stereo, (const float *)(db + L.X), (const float *)(db + L.uv),
        stereo ? (const float *)(db + L.uvr) : nullptr, n, fx, fy, cx, cy, *p3, dT, db + L.mask,
        stereo ? db + L.maskr : nullptr, opt->threshold_huber_loss, opt->threshold_step_size,
        opt->threshold_cost_change, opt->threshold_outlier_rejection, max_it,
        (ba::PoIter *)(db + L.iters), icap, (int *)(db + L.meta), ddbg, (int *)(db + L.gsw),
        h->po_part, s);
  else if (stereo)
    rc = ba::pose_only_stereo6_device(
        (const float *)(db + L.X), (const float *)(db + L.uv), (const float *)(db + L.uvr), n, fx, fy,
        cx, cy, (const float *)(db + L.camr), dT, db + L.mask, db + L.maskr, opt->threshold_huber_loss,
        opt->threshold_step_size, opt->threshold_cost_change, opt->threshold_outlier_rejection, max_it,
        (ba::PoIter *)(db + L.iters), icap, (int *)(db + L.meta), ddbg, (int *)(db + L.gsw), h->po_part, s);
  else
    rc = ba::pose_only_mono6_device(
        (const float *)(db + L.X), (const float *)(db + L.uv), n, fx, fy, cx, cy, dT, db + L.mask,
        opt->threshold_huber_loss, opt->threshold_step_size, opt->threshold_cost_change,
        opt->threshold_outlier_rejection, max_it, (ba::PoIter *)(db + L.iters), icap,
        (int *)(db + L.meta), ddbg, (int *)(db + L.gsw), h->po_part, s);
  if (rc) return fail("pose-only kernel launch failed");
  HIP_TRY(hipMemcpyAsync(hb + L.T, db + L.T, L.end - L.T, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  int meta[4], gsw[2];
  std::memcpy(meta, hb + L.meta, sizeof(meta));
  std::memcpy(gsw, hb + L.gsw, sizeof(gsw));
  if (gsw[1]) return fail("pose-only kernel: grid barrier timed out");
  std::memcpy(T12, hb + L.T, 12 * sizeof(float));
  std::memcpy(mask, hb + L.mask, (size_t)n);
  if (stereo) std::memcpy(mask_r, hb + L.maskr, (size_t)n);
  if (max_it <= 0) { meta[0] = 0; meta[1] = 1; meta[2] = 0; meta[3] = 1; }
  const int rows = std::min(meta[2], cap);
  if (iters && rows > 0) std::memcpy(iters, hb + L.iters, (size_t)rows * sizeof(ba_po_iter));
  if (debug_T12 && meta[0] > 0)
    std::memcpy(debug_T12, hb + L.dbg, (size_t)std::min(meta[0], cap) * 12 * sizeof(float));
  if (n_iter) *n_iter = meta[0];
  if (converged) *converged = meta[1];
  return meta[3] ? 0 : 1;  // 1 = NaN pose, input left unchanged (reference :159-167)
}
}  // namespace

extern "C" {

int ba_pose_only_mono6(ba_handle *h, const float *X3, const float *uv2, int n,
                       float fx, float fy, float cx, float cy, float *T12,
                       uint8_t *mask, const ba_options *opt, ba_po_iter *iters,
                       int cap, int *n_iter, int *converged,
                       float *debug_T12) {
  if (!h || !X3 || !uv2 || n <= 0 || !T12 || !mask || !opt)
    return fail("ba_pose_only_mono6: bad argument");
  return po_run(h, false, X3, uv2, nullptr, n, fx, fy, cx, cy, nullptr, T12, mask, nullptr, opt,
                iters, cap, n_iter, converged, debug_T12);
}

int ba_pose_only_stereo6(ba_handle *h, const float *X3, const float *uv2,
                         const float *uvr2, int n, const float *intr_l4,
                         const float *intr_r4, const float *T_lr12, float *T12,
                         uint8_t *mask, uint8_t *mask_r, const ba_options *opt,
                         ba_po_iter *iters, int cap, int *n_iter, int *converged,
                         float *debug_T12) {
  if (!h || !X3 || !uv2 || !uvr2 || n <= 0 || !intr_l4 || !intr_r4 || !T_lr12 || !T12 ||
      !mask || !mask_r || !opt)
    return fail("ba_pose_only_stereo6: bad argument");
  float camr[16];
  po_right_camera(intr_r4, T_lr12, camr);
  return po_run(h, true, X3, uv2, uvr2, n, intr_l4[0], intr_l4[1], intr_l4[2], intr_l4[3], camr, T12,
                mask, mask_r, opt, iters, cap, n_iter, converged, debug_T12);
}

// ---- planar 3-DoF (reference :401-900) ----------------------------------------
namespace {
// fp32 rigid transforms in the reference's Eigen operation order: R (9,
// row-major) then t (3), like the 12-float ABI poses
struct Iso {
  float R[9], t[3];
};
Iso iso12(const float *T12) {
  Iso A;
  for (int k = 0; k < 9; ++k) A.R[k] = T12[k];
  for (int k = 0; k < 3; ++k) A.t[k] = T12[9 + k];
  return A;
}
Iso iso_mul(const Iso &A, const Iso &B) {
  Iso C;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      C.R[r * 3 + c] = A.R[r * 3 + 0] * B.R[0 * 3 + c] + A.R[r * 3 + 1] * B.R[1 * 3 + c] +
                       A.R[r * 3 + 2] * B.R[2 * 3 + c];
    C.t[r] = (A.R[r * 3 + 0] * B.t[0] + A.R[r * 3 + 1] * B.t[1] + A.R[r * 3 + 2] * B.t[2]) + A.t[r];
  }
  return C;
}
Iso iso_inv(const Iso &A) {
  Iso B;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) B.R[r * 3 + c] = A.R[c * 3 + r];
  for (int r = 0; r < 3; ++r)
    B.t[r] = -(B.R[r * 3 + 0] * A.t[0] + B.R[r * 3 + 1] * A.t[1] + B.R[r * 3 + 2] * A.t[2]);
  return B;
}
// the host-side set-up of both planar solvers (reference :446-460 / :674-692)
ba::Po3Params po3_params(const float *T_bc12, const float *T_wl12, const float *T12,
                         const float *T_lr12, const float *intr_r4) {
  ba::Po3Params P;
  const Iso Tbc = iso12(T_bc12), Tcb = iso_inv(Tbc);
  const Iso prior = iso_mul(iso_inv(iso12(T12)), iso12(T_wl12));   // pose_c2c1_prior
  const Iso Pb = iso_mul(iso_mul(Tbc, prior), Tcb);                 // pose_b2b1
  P.theta0[0] = Pb.t[0];
  P.theta0[1] = Pb.t[1];
  P.theta0[2] = std::atan2(Pb.R[3], Pb.R[0]);
  std::memcpy(P.Rcb, Tcb.R, sizeof(P.Rcb));
  std::memcpy(P.tcb, Tcb.t, sizeof(P.tcb));
  std::memcpy(P.Rbc, Tbc.R, sizeof(P.Rbc));
  std::memcpy(P.tbc, Tbc.t, sizeof(P.tbc));
  Iso Trl{};
  if (T_lr12) Trl = iso_inv(iso12(T_lr12));
  std::memcpy(P.Rrl, Trl.R, sizeof(P.Rrl));
  std::memcpy(P.trl, Trl.t, sizeof(P.trl));
  const Iso Rrb = iso_mul(Trl, Tcb);  // only its rotation is used: R_rl * R_cb
  std::memcpy(P.Rrb, Rrb.R, sizeof(P.Rrb));
  for (int k = 0; k < 4; ++k) P.cam_r[k] = intr_r4 ? intr_r4[k] : 0.0f;
  return P;
}
}  // namespace

int ba_pose_only_mono3(ba_handle *h, const float *X3, const float *uv2, int n,
                       float fx, float fy, float cx, float cy,
                       const float *T_bc12, const float *T_wl12, float *T12,
                       uint8_t *mask, const ba_options *opt, ba_po_iter *iters,
                       int cap, int *n_iter, int *converged,
                       float *debug_T12) {
  if (!h || !X3 || !uv2 || n <= 0 || !T_bc12 || !T_wl12 || !T12 || !mask || !opt)
    return fail("ba_pose_only_mono3: bad argument");
  const ba::Po3Params P = po3_params(T_bc12, T_wl12, T12, nullptr, nullptr);
  return po_run(h, false, X3, uv2, nullptr, n, fx, fy, cx, cy, nullptr, T12, mask, nullptr, opt,
                iters, cap, n_iter, converged, debug_T12, &P);
}

int ba_pose_only_stereo3(ba_handle *h, const float *X3, const float *uvl2,
                         const float *uvr2, int n, const float *intr_l4,
                         const float *intr_r4, const float *T_bc12,
                         const float *T_lr12, const float *T_wl12, float *T12,
                         uint8_t *mask_l, uint8_t *mask_r, const ba_options *opt,
                         ba_po_iter *iters, int cap, int *n_iter, int *converged,
                         float *debug_T12) {
  if (!h || !X3 || !uvl2 || !uvr2 || n <= 0 || !intr_l4 || !intr_r4 || !T_bc12 || !T_lr12 ||
      !T_wl12 || !T12 || !mask_l || !mask_r || !opt)
    return fail("ba_pose_only_stereo3: bad argument");
  const ba::Po3Params P = po3_params(T_bc12, T_wl12, T12, T_lr12, intr_r4);
  return po_run(h, true, X3, uvl2, uvr2, n, intr_l4[0], intr_l4[1], intr_l4[2], intr_l4[3],
                nullptr, T12, mask_l, mask_r, opt, iters, cap, n_iter, converged, debug_T12, &P);
}

}  // extern "C"

// ---- batched pose-only, 6-DoF and planar 3-DoF (one workgroup per problem) ---
namespace {
// one pinned staging buffer mirroring one device buffer, as po_run:
//   [offsets | X | uv | uv_right | intrinsics | records | T | mask | mask_right]  <- H2D
//                                          [ T | mask | mask_right | results | iters | debug ]  <- D2H
// records: rec_floats per problem (6-DoF stereo: the 16-float right cameras,
// 6-DoF mono: none, planar: the 52-float Po3Params)
struct PoBatchLayout {
  size_t off, X, uv, uvr, intr, rec, T, mask, maskr, h2d_end, res, iters, dbg, end;
};
PoBatchLayout po_batch_layout(int B, int64_t N, int cap, bool stereo, int rec_floats, bool want_iters,
                              bool want_dbg) {
  auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
  PoBatchLayout L;
  size_t o = 0;
  L.off = o;    o = al(o + (size_t)(B + 1) * sizeof(int32_t));
  L.X = o;      o = al(o + (size_t)N * 3 * sizeof(float));
  L.uv = o;     o = al(o + (size_t)N * 2 * sizeof(float));
  L.uvr = o;    o = al(o + (stereo ? (size_t)N * 2 * sizeof(float) : 0));
  L.intr = o;   o = al(o + (size_t)B * 4 * sizeof(float));
  L.rec = o;    o = al(o + (size_t)B * rec_floats * sizeof(float));
  L.T = o;      o = al(o + (size_t)B * 12 * sizeof(float));
  L.mask = o;   o = al(o + (size_t)N);
  L.maskr = o;  o = al(o + (stereo ? (size_t)N : 0));
  L.h2d_end = o;
  L.res = o;    o = al(o + (size_t)B * sizeof(ba_po_result));
  L.iters = o;  o = al(o + (want_iters ? (size_t)B * cap * sizeof(ba_po_iter) : 0));
  L.dbg = o;    o = al(o + (want_dbg ? (size_t)B * cap * 12 * sizeof(float) : 0));
  L.end = o;
  return L;
}

// host-side checks shared by both host-array entry points (nothing runs on failure)
int po_batch_check(const char *fn, ba_handle *h, int B, const int32_t *offsets, int cap) {
  const std::string f(fn);
  if (B < 1) return fail(f + ": B must be >= 1");
  if (!offsets) return fail(f + ": null offsets");
  if (offsets[0] != 0) return fail(f + ": offsets[0] must be 0");
  for (int b = 0; b < B; ++b)
    if (offsets[b + 1] <= offsets[b])
      return fail(f + ": offsets must be strictly increasing (problem " + std::to_string(b) + ")");
  if (cap < 0) return fail(f + ": cap must be >= 0");
  if (!h) return fail(f + ": null handle");
  return 0;
}

// planar: the records come from T_bc12 / T_wl12 / T12 (and T_lr12 / intr_r4 in
// stereo) through po3_params, as in the single calls; 6-DoF stereo: the right
// cameras from intr_r4 / T_lr12
int po_batch_run(const char *fn, ba_handle *h, bool stereo, bool planar, int B, const int32_t *offsets,
                 const float *X3, const float *uvl2, const float *uvr2, const float *intr_l4,
                 const float *intr_r4, const float *T_lr12, const float *T_bc12, const float *T_wl12,
                 float *T12, uint8_t *mask_l, uint8_t *mask_r, const ba_options *opt,
                 ba_po_iter *iters, int cap, ba_po_result *res, float *debug_T12) {
  if (use_device(h)) return -1;
  const int64_t N = offsets[B];
  const bool want_it = iters && cap > 0, want_dbg = debug_T12 && cap > 0;
  constexpr int kRec3 = sizeof(ba::Po3Params) / sizeof(float);
  const int rec_floats = planar ? kRec3 : (stereo ? 16 : 0);
  const PoBatchLayout L = po_batch_layout(B, N, cap, stereo, rec_floats, want_it, want_dbg);
  if (po_reserve(h, L.end)) return -1;
  uint8_t *hb = h->po_host, *db = h->po_dev;
  std::memcpy(hb + L.off, offsets, (size_t)(B + 1) * sizeof(int32_t));
  std::memcpy(hb + L.X, X3, (size_t)N * 3 * sizeof(float));
  std::memcpy(hb + L.uv, uvl2, (size_t)N * 2 * sizeof(float));
  std::memcpy(hb + L.intr, intr_l4, (size_t)B * 4 * sizeof(float));
  std::memcpy(hb + L.T, T12, (size_t)B * 12 * sizeof(float));
  std::memcpy(hb + L.mask, mask_l, (size_t)N);
  float *rec = (float *)(hb + L.rec);
  if (planar) {
    for (int b = 0; b < B; ++b) {
      const ba::Po3Params P = po3_params(T_bc12 + 12 * b, T_wl12 + 12 * b, T12 + 12 * b,
                                         stereo ? T_lr12 + 12 * b : nullptr,
                                         stereo ? intr_r4 + 4 * b : nullptr);
      std::memcpy(rec + (size_t)kRec3 * b, &P, sizeof(P));
    }
  } else if (stereo) {
    for (int b = 0; b < B; ++b) po_right_camera(intr_r4 + 4 * b, T_lr12 + 12 * b, rec + 16 * b);
  }
  if (stereo) {
    std::memcpy(hb + L.uvr, uvr2, (size_t)N * 2 * sizeof(float));
    std::memcpy(hb + L.maskr, mask_r, (size_t)N);
  }
  hipStream_t s = h->stream;
  HIP_TRY(hipMemcpyAsync(db, hb, L.h2d_end, hipMemcpyHostToDevice, s));
  ba_po_iter *dit = want_it ? (ba_po_iter *)(db + L.iters) : nullptr;
  float *ddbg = want_dbg ? (float *)(db + L.dbg) : nullptr;
  const int32_t *doff = (const int32_t *)(db + L.off);
  ba_po_result *dres = (ba_po_result *)(db + L.res);
  const float *dX = (const float *)(db + L.X), *duv = (const float *)(db + L.uv);
  const float *duvr = (const float *)(db + L.uvr), *dintr = (const float *)(db + L.intr);
  const float *drec = (const float *)(db + L.rec);
  float *dT = (float *)(db + L.T);
  int rc;
  if (planar)
    rc = stereo ? ba_pose_only_stereo3_batch_device(h, B, doff, dX, duv, duvr, dintr, drec, dT,
                                                    db + L.mask, db + L.maskr, opt, dit, cap, dres,
                                                    ddbg, (void *)s)
                : ba_pose_only_mono3_batch_device(h, B, doff, dX, duv, dintr, drec, dT, db + L.mask,
                                                  opt, dit, cap, dres, ddbg, (void *)s);
  else
    rc = stereo ? ba_pose_only_stereo6_batch_device(h, B, doff, dX, duv, duvr, dintr, drec, dT,
                                                    db + L.mask, db + L.maskr, opt, dit, cap, dres,
                                                    ddbg, (void *)s)
                : ba_pose_only_mono6_batch_device(h, B, doff, dX, duv, dintr, dT, db + L.mask, opt,
                                                  dit, cap, dres, ddbg, (void *)s);
  if (rc) return fail(std::string(fn) + ": " + g_err);
  HIP_TRY(hipMemcpyAsync(hb + L.T, db + L.T, L.end - L.T, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const ba_po_result *hr = (const ba_po_result *)(hb + L.res);
  std::memcpy(T12, hb + L.T, (size_t)B * 12 * sizeof(float));  // unchanged where not written
  std::memcpy(mask_l, hb + L.mask, (size_t)N);
  if (stereo) std::memcpy(mask_r, hb + L.maskr, (size_t)N);
  if (res) std::memcpy(res, hr, (size_t)B * sizeof(ba_po_result));
  for (int b = 0; b < B; ++b) {
    const int rows = std::min(hr[b].n_rows, cap), its = std::min(hr[b].n_iter, cap);
    if (want_it && rows > 0)
      std::memcpy(iters + (size_t)b * cap, hb + L.iters + (size_t)b * cap * sizeof(ba_po_iter),
                  (size_t)rows * sizeof(ba_po_iter));
    if (want_dbg && its > 0)
      std::memcpy(debug_T12 + (size_t)b * cap * 12, hb + L.dbg + (size_t)b * cap * 12 * sizeof(float),
                  (size_t)its * 12 * sizeof(float));
  }
  return 0;
}
}  // namespace

extern "C" {

int ba_pose_only_mono6_batch_device(ba_handle *h, int B, const int32_t *offsets, const float *X3,
                                    const float *uv2, const float *intr4, float *T12, uint8_t *mask,
                                    const ba_options *opt, ba_po_iter *iters, int cap,
                                    ba_po_result *res, float *debug_T12, void *hip_stream) {
  if (!h || B < 1 || !offsets || !X3 || !uv2 || !intr4 || !T12 || !mask || !opt || !res || cap < 0)
    return fail("ba_pose_only_mono6_batch_device: bad argument");
  if (use_device(h)) return -1;
  static_assert(sizeof(ba::PoIter) == sizeof(ba_po_iter), "po iter layout");
  static_assert(sizeof(ba_po_result) == 4 * sizeof(int), "po result layout");
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
  if (ba::pose_only6_batch_device(false, B, offsets, X3, uv2, nullptr, intr4, nullptr, T12, mask,
                                  nullptr, opt->threshold_huber_loss, opt->threshold_step_size,
                                  opt->threshold_cost_change, opt->threshold_outlier_rejection,
                                  opt->max_num_iterations, cap > 0 ? (ba::PoIter *)iters : nullptr,
                                  cap, (int *)res, cap > 0 ? debug_T12 : nullptr, s))
    return fail("ba_pose_only_mono6_batch_device: kernel launch failed");
  return 0;
}

int ba_pose_only_stereo6_batch_device(ba_handle *h, int B, const int32_t *offsets, const float *X3,
                                      const float *uvl2, const float *uvr2, const float *intr_l4,
                                      const float *camr16, float *T12, uint8_t *mask_l,
                                      uint8_t *mask_r, const ba_options *opt, ba_po_iter *iters,
                                      int cap, ba_po_result *res, float *debug_T12,
                                      void *hip_stream) {
  if (!h || B < 1 || !offsets || !X3 || !uvl2 || !uvr2 || !intr_l4 || !camr16 || !T12 || !mask_l ||
      !mask_r || !opt || !res || cap < 0)
    return fail("ba_pose_only_stereo6_batch_device: bad argument");
  if (use_device(h)) return -1;
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
  if (ba::pose_only6_batch_device(true, B, offsets, X3, uvl2, uvr2, intr_l4, camr16, T12, mask_l,
                                  mask_r, opt->threshold_huber_loss, opt->threshold_step_size,
                                  opt->threshold_cost_change, opt->threshold_outlier_rejection,
                                  opt->max_num_iterations, cap > 0 ? (ba::PoIter *)iters : nullptr,
                                  cap, (int *)res, cap > 0 ? debug_T12 : nullptr, s))
    return fail("ba_pose_only_stereo6_batch_device: kernel launch failed");
  return 0;
}

int ba_right_camera_record(const float *intr_r4, const float *T_lr12, float *camr16) {
  if (!intr_r4 || !T_lr12 || !camr16) return fail("ba_right_camera_record: bad argument");
  po_right_camera(intr_r4, T_lr12, camr16);
  return 0;
}

int ba_pose_only_mono6_batch(ba_handle *h, int B, const int32_t *offsets, const float *X3,
                             const float *uv2, const float *intr4, float *T12, uint8_t *mask,
                             const ba_options *opt, ba_po_iter *iters, int cap, ba_po_result *res,
                             float *debug_T12) {
  const char *fn = "ba_pose_only_mono6_batch";
  if (po_batch_check(fn, h, B, offsets, cap)) return -1;
  if (!X3 || !uv2 || !intr4 || !T12 || !mask || !opt || !res)
    return fail(std::string(fn) + ": bad argument");
  return po_batch_run(fn, h, false, false, B, offsets, X3, uv2, nullptr, intr4, nullptr, nullptr,
                      nullptr, nullptr, T12, mask, nullptr, opt, iters, cap, res, debug_T12);
}

int ba_pose_only_stereo6_batch(ba_handle *h, int B, const int32_t *offsets, const float *X3,
                               const float *uvl2, const float *uvr2, const float *intr_l4,
                               const float *intr_r4, const float *T_lr12, float *T12,
                               uint8_t *mask_l, uint8_t *mask_r, const ba_options *opt,
                               ba_po_iter *iters, int cap, ba_po_result *res, float *debug_T12) {
  const char *fn = "ba_pose_only_stereo6_batch";
  if (po_batch_check(fn, h, B, offsets, cap)) return -1;
  if (!X3 || !uvl2 || !uvr2 || !intr_l4 || !intr_r4 || !T_lr12 || !T12 || !mask_l || !mask_r || !opt ||
      !res)
    return fail(std::string(fn) + ": bad argument");
  return po_batch_run(fn, h, true, false, B, offsets, X3, uvl2, uvr2, intr_l4, intr_r4, T_lr12,
                      nullptr, nullptr, T12, mask_l, mask_r, opt, iters, cap, res, debug_T12);
}

// ---- batched planar 3-DoF -----------------------------------------------------
int ba_planar_record(const float *T_bc12, const float *T_wl12, const float *T12,
                     const float *T_lr12, const float *intr_r4, float *rec52) {
  if (!T_bc12 || !T_wl12 || !T12 || !rec52 || (!T_lr12) != (!intr_r4))
    return fail("ba_planar_record: bad argument");
  const ba::Po3Params P = po3_params(T_bc12, T_wl12, T12, T_lr12, intr_r4);
  std::memcpy(rec52, &P, sizeof(P));
  return 0;
}

int ba_pose_only_mono3_batch_device(ba_handle *h, int B, const int32_t *offsets, const float *X3,
                                    const float *uv2, const float *intr4, const float *rec52,
                                    float *T12, uint8_t *mask, const ba_options *opt,
                                    ba_po_iter *iters, int cap, ba_po_result *res, float *debug_T12,
                                    void *hip_stream) {
  if (!h || B < 1 || !offsets || !X3 || !uv2 || !intr4 || !rec52 || !T12 || !mask || !opt || !res ||
      cap < 0)
    return fail("ba_pose_only_mono3_batch_device: bad argument");
  if (use_device(h)) return -1;
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
  if (ba::pose_only3_batch_device(false, B, offsets, X3, uv2, nullptr, intr4, rec52, T12, mask,
                                  nullptr, opt->threshold_huber_loss, opt->threshold_step_size,
                                  opt->threshold_cost_change, opt->threshold_outlier_rejection,
                                  opt->max_num_iterations, cap > 0 ? (ba::PoIter *)iters : nullptr,
                                  cap, (int *)res, cap > 0 ? debug_T12 : nullptr, s))
    return fail("ba_pose_only_mono3_batch_device: kernel launch failed");
  return 0;
}

int ba_pose_only_stereo3_batch_device(ba_handle *h, int B, const int32_t *offsets, const float *X3,
                                      const float *uvl2, const float *uvr2, const float *intr_l4,
                                      const float *rec52, float *T12, uint8_t *mask_l,
                                      uint8_t *mask_r, const ba_options *opt, ba_po_iter *iters,
                                      int cap, ba_po_result *res, float *debug_T12,
                                      void *hip_stream) {
  if (!h || B < 1 || !offsets || !X3 || !uvl2 || !uvr2 || !intr_l4 || !rec52 || !T12 || !mask_l ||
      !mask_r || !opt || !res || cap < 0)
    return fail("ba_pose_only_stereo3_batch_device: bad argument");
  if (use_device(h)) return -1;
  hipStream_t s = hip_stream ? (hipStream_t)hip_stream : h->stream;
  if (ba::pose_only3_batch_device(true, B, offsets, X3, uvl2, uvr2, intr_l4, rec52, T12, mask_l,
                                  mask_r, opt->threshold_huber_loss, opt->threshold_step_size,
                                  opt->threshold_cost_change, opt->threshold_outlier_rejection,
                                  opt->max_num_iterations, cap > 0 ? (ba::PoIter *)iters : nullptr,
                                  cap, (int *)res, cap > 0 ? debug_T12 : nullptr, s))
    return fail("ba_pose_only_stereo3_batch_device: kernel launch failed");
  return 0;
}

int ba_pose_only_mono3_batch(ba_handle *h, int B, const int32_t *offsets, const float *X3,
                             const float *uv2, const float *intr4, const float *T_bc12,
                             const float *T_wl12, float *T12, uint8_t *mask, const ba_options *opt,
                             ba_po_iter *iters, int cap, ba_po_result *res, float *debug_T12) {
  const char *fn = "ba_pose_only_mono3_batch";
  if (po_batch_check(fn, h, B, offsets, cap)) return -1;
  if (!X3 || !uv2 || !intr4 || !T_bc12 || !T_wl12 || !T12 || !mask || !opt || !res)
    return fail(std::string(fn) + ": bad argument");
  return po_batch_run(fn, h, false, true, B, offsets, X3, uv2, nullptr, intr4, nullptr, nullptr,
                      T_bc12, T_wl12, T12, mask, nullptr, opt, iters, cap, res, debug_T12);
}

int ba_pose_only_stereo3_batch(ba_handle *h, int B, const int32_t *offsets, const float *X3,
                               const float *uvl2, const float *uvr2, const float *intr_l4,
                               const float *intr_r4, const float *T_bc12, const float *T_lr12,
                               const float *T_wl12, float *T12, uint8_t *mask_l, uint8_t *mask_r,
                               const ba_options *opt, ba_po_iter *iters, int cap, ba_po_result *res,
                               float *debug_T12) {
  const char *fn = "ba_pose_only_stereo3_batch";
  if (po_batch_check(fn, h, B, offsets, cap)) return -1;
  if (!X3 || !uvl2 || !uvr2 || !intr_l4 || !intr_r4 || !T_bc12 || !T_lr12 || !T_wl12 || !T12 ||
      !mask_l || !mask_r || !opt || !res)
    return fail(std::string(fn) + ": bad argument");
  return po_batch_run(fn, h, true, true, B, offsets, X3, uvl2, uvr2, intr_l4, intr_r4, T_lr12,
                      T_bc12, T_wl12, T12, mask_l, mask_r, opt, iters, cap, res, debug_T12);
}

}  // extern "C"
