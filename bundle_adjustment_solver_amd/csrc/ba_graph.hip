// ba_graph.hip — the host driver of the pose graphs (ba_graph.h): creation
// and the device set-up, the LM loop, the passes outside it, the robust arrays, and the
// covariance / gate driver (§6m, §6p), once for the SE(3) graph (ba_pgraph_*) and the Sim(3) graph
// (ba_sim3_*).  Host code only: the kernels and their launchers are in ba_graph_kernels.hip, and
// reach this file through the GraphSpec of a kind (ba_pgraph.hip, ba_sim3.hip).
#include <cstddef>
#include <cstring>

#include "ba_graph.h"

namespace ba {
namespace {

int push_ctrl(GraphHost *g) {
  HIP_TRY(hipMemcpyAsync(g->d.ctrl, &g->hc, sizeof(ba::PgCtrl), hipMemcpyHostToDevice, g->h->stream));
  return 0;
}
int pull_ctrl(GraphHost *g) {
  HIP_TRY(hipMemcpyAsync(&g->hc, g->d.ctrl, sizeof(ba::PgCtrl), hipMemcpyDeviceToHost, g->h->stream));
  HIP_TRY(hipStreamSynchronize(g->h->stream));
  return 0;
}
const int *done_flag(const GraphHost *g) {
  return (const int *)((const char *)g->d.ctrl + offsetof(PgCtrl, done));
}

void free_device(GraphHost *g) {
  for (void *p : g->allocs) (void)hipFree(p);
  g->allocs.clear();
  if (g->e0) (void)hipEventDestroy(g->e0);
  if (g->e1) (void)hipEventDestroy(g->e1);
  g->e0 = g->e1 = nullptr;
}

// the device side of a validated graph; on failure the caller frees what `g` holds
int build_device(const GraphSpec &k, GraphHost *g, const double *poses) {
  ba_handle *h = g->h;
  const PgraphLists &l = g->lists;
  const DenseKnobs &knobs = h->knobs.dense;
  PgDev &d = g->d;
  const int N = l.N, W = k.W;
  // both tile orders, as ba_finalize builds them for the reduced camera system
  DenseSchedule cand[2];
  const int orders[2] = {32, 64};
  for (int o = 0; o < 2; ++o) {
    int ncb_o = 0;
    std::vector<uint8_t> adj;
    pgraph_tile_adjacency(l, k.poses_per_tile(orders[o]), &ncb_o, &adj);
    if (knobs.full) std::fill(adj.begin(), adj.end(), 1);
    build_dense_schedule(ncb_o, adj, knobs.natural, orders[o], cand[o], knobs.order);
  }
  g->sched = cand[dense_pick_tile_order(cand[0], cand[1], knobs.nb)];
  const DenseSchedule &sc = g->sched;
  const int nb = sc.nb, ppt = k.poses_per_tile(nb), ncb = sc.ncb;
  g->nb = nb;
  g->ncb = ncb;
  d.n_pose = g->n_pose;
  d.N = N;
  d.F = (int)g->F;
  d.nblk = (int)(l.blk.size() / 2);
  d.n_part = (int)((g->F + k.fpb - 1) / k.fpb);
  d.n_tpart = (N + 255) / 256;
  d.npad = ncb * nb;
  d.ld = d.npad + nb;
  d.log_cap = 4096;
  // the image first: nothing is launched, and nothing else allocated, if it does not fit
  g->image_bytes = (size_t)d.npad * d.ld * sizeof(double);
  {
    hipError_t e = hipMalloc((void **)&d.L, g->image_bytes);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      d.L = nullptr;
      return fail(std::string(k.abi) + "_create: cannot allocate the dense image of " + std::to_string(d.npad) +
                  " x " + std::to_string(d.ld) + " doubles (" + std::to_string(g->image_bytes) + " bytes): " +
                  hipGetErrorString(e));
    }
    g->allocs.push_back((void *)d.L);
  }
  // W columns per pose; the nb - W ppt columns at the end of a tile are padding (col_x < 0:
  // k_dense_init gives them a unit diagonal)
  std::vector<int> pose_col((size_t)N, 0), col_x((size_t)d.npad, -1);
  for (int j = 0; j < N; ++j) {
    const int c0 = sc.pos_of_tile[j / ppt] * nb + W * (j % ppt);
    pose_col[j] = c0;
    for (int r = 0; r < W; ++r) col_x[c0 + r] = W * j + r;
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
  g->n_zt = (int)ztI.size();
  g->pose_col_h = pose_col;
  std::vector<double> val;
  k.pack_values(g->F, g->Z.data(), g->Om.data(), &val);
  constexpr Mem R = Mem::Resident;
  static_assert(sizeof(int4) == 16 && sizeof(int2) == 8, "layout");
  int4 *jk = nullptr;
  int2 *blk = nullptr;
  int32_t *pptr = nullptr, *plist = nullptr, *bptr = nullptr, *blist = nullptr, *opt_pose = nullptr;
  int *pc = nullptr;
  const size_t nW = (size_t)W * N, n_rec = (size_t)g->F * k.rec_doubles;
  const size_t n_poses = (size_t)g->n_pose * k.pose_doubles;
  if (upload_dense_schedule(h, sc, col_x, g->dd) ||
      h->dalloc(R, &g->Ldiag, (size_t)ncb * dense_ws_per_block(nb)) || h->upload(R, &pc, pose_col) ||
      h->upload(R, &g->zt_I, ztI) || h->upload(R, &g->zt_J, ztJ) || h->upload(R, &d.poses[0], poses, n_poses) ||
      h->upload(R, &d.poses[1], poses, n_poses) || h->upload(R, &jk, l.jk.data(), (size_t)g->F) ||
      h->upload(R, &g->val, val) || h->upload(R, &pptr, l.pptr) || h->upload(R, &plist, l.plist) ||
      h->upload(R, &blk, l.blk.data(), l.blk.size() / 2) || h->upload(R, &bptr, l.bptr) ||
      h->upload(R, &blist, l.blist) || h->upload(R, &opt_pose, l.opt_pose) || h->dalloc(R, &d.rec, n_rec) ||
      h->dalloc(R, &d.dH, nW) || h->dalloc(R, &d.g, nW) || h->dalloc(R, &d.x, nW + 64) ||
      h->dalloc(R, &d.part[0], (size_t)d.n_part) || h->dalloc(R, &d.part[1], (size_t)d.n_part) ||
      h->dalloc(R, &d.tpart, (size_t)2 * d.n_tpart) || h->dalloc(R, &d.ctrl, (size_t)1) ||
      h->dalloc(R, &d.log, (size_t)d.log_cap))
    return -1;
  g->col_x = g->dd.col_x;
  d.jk = jk;
  d.val = g->val;
  d.pptr = pptr;
  d.plist = plist;
  d.blk = blk;
  d.bptr = bptr;
  d.blist = blist;
  d.opt_pose = opt_pose;
  d.pose_col = pc;
  HIP_TRY(hipMemset(d.L, 0, g->image_bytes));
  HIP_TRY(hipMemset(d.rec, 0, n_rec * sizeof(double)));
  HIP_TRY(hipMemset(d.dH, 0, nW * sizeof(double)));
  HIP_TRY(hipMemset(d.g, 0, nW * sizeof(double)));
  HIP_TRY(hipMemset(d.x, 0, (nW + 64) * sizeof(double)));
  HIP_TRY(hipMemset(d.part[0], 0, (size_t)d.n_part * sizeof(double)));
  HIP_TRY(hipMemset(d.part[1], 0, (size_t)d.n_part * sizeof(double)));
  HIP_TRY(hipMemset(d.tpart, 0, (size_t)2 * d.n_tpart * sizeof(double)));
  HIP_TRY(hipMemset(d.ctrl, 0, sizeof(ba::PgCtrl)));
  HIP_TRY(hipEventCreate(&g->e0));
  HIP_TRY(hipEventCreate(&g->e1));
  return 0;
}

// the device arrays of the robust kernels: kinds 0 and the weights' arrays, once per graph
int ensure_robust_arrays(GraphHost *g) {
  if (g->d_rkind) return 0;
  ba_handle *h = g->h;
  constexpr Mem R = Mem::Resident;
  const size_t F = (size_t)g->F, mark = h->allocs.size();
  const int rc = h->dalloc(R, &g->d_rkind, F) || h->dalloc(R, &g->d_rscale, F) || h->dalloc(R, &g->rb.s, F) ||
                 h->dalloc(R, &g->rb.w, F) || h->dalloc(R, &g->d_rep_s, F) || h->dalloc(R, &g->d_rep_w, F);
  graph_adopt_allocs(g, mark);
  if (rc) {
    g->d_rkind = nullptr;  // what was allocated goes with the graph
    return -1;
  }
  g->rb.kind = g->d_rkind;
  g->rb.scale = g->d_rscale;
  HIP_TRY(hipMemset(g->d_rkind, 0, F * sizeof(int32_t)));
  HIP_TRY(hipMemset(g->d_rscale, 0, F * sizeof(double)));
  return 0;
}

// the linearisation / cost pass and the assembly of the graph: the robust kernels only where
// one is set
void lin(const GraphSpec &k, const GraphHost *g, int cost_only, hipStream_t s) {
  if (g->robust)
    k.lin_robust(g->d, g->rb, cost_only, s);
  else
    k.lin(g->d, cost_only, s);
}
void assemble(const GraphSpec &k, const GraphHost *g, double *Hout, double *gout, hipStream_t s) {
  if (g->robust)
    k.assemble_robust(g->d, g->rb, Hout, gout, s);
  else
    k.assemble(g->d, Hout, gout, s);
}

template <class T>
int download(std::vector<T> &out, const T *dev, size_t n, hipStream_t s) {
  out.resize(n);
  if (n) HIP_TRY(hipMemcpyAsync(out.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
  return 0;
}

// The host arrays of one covariance or gate call (validated): entry_kind = kPgCovPair with
// Z = Omega = nullptr, or kPgCovCand.  Outputs that are null are not produced.
struct GraphCovCall {
  int n_pose_sel = 0;
  const int32_t *pose_sel = nullptr;
  double *cov_pose = nullptr;
  int64_t n_entry = 0;
  int entry_kind = kPgCovPair;
  const int32_t *entry_j = nullptr, *entry_k = nullptr;
  const double *Z = nullptr, *Omega = nullptr;
  double *cov_cross = nullptr, *cov_rel = nullptr, *d2 = nullptr, *r = nullptr, *innov = nullptr;
};

// Factorise H at lambda = 0 at the accepted poses with the solve's launches, sweep the groups
// in column batches, copy the blocks out.  The controller, the solve's count of dropped pivots
// and last_ms are as before on return; the workspace and the lists are freed on every path.
int graph_cov_run(const GraphSpec &k, GraphHost *g, const std::string &what, const GraphCovCall &c,
                  int64_t *dropped_pivots) {
  ba_handle *h = g->h;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const PgDev &d = g->d;
  const DenseSchedule &sc = g->sched;
  const size_t W = (size_t)k.W, WW = W * W;
  std::vector<PgCovGroup> groups;
  std::vector<int32_t> slot_of_opt;
  int n_pose_rows = 0;
  pgraph_cov_groups(g->lists, g->pose_col_h, g->nb, c.n_pose_sel, c.pose_sel, c.n_entry, c.entry_j, c.entry_k,
                    c.entry_kind, &groups, &slot_of_opt, &n_pose_rows);
  std::vector<int> trow_ptr, trow;
  pgraph_cov_tile_rows(g->ncb, sc.row_ptr, sc.rows, &trow_ptr, &trow);
  // ---- the factor of H at lambda = 0, whole in the image (no level goes to k_chol_tail)
  HIP_TRY(hipStreamSynchronize(s));
  const PgCtrl keep = g->hc;
  int bad_keep = 0, bad_now = 0;
  HIP_TRY(hipMemcpy(&bad_keep, g->dd.bad_pivots, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemsetAsync(g->dd.bad_pivots, 0, sizeof(int), s));
  if (graph_begin_pass(g)) return -1;
  const int *done = done_flag(g);
  lin(k, g, 0, s);
  launch_dense_init(d.L, d.ld, g->col_x, g->zt_I, g->zt_J, g->n_zt, g->nb, done, s);
  assemble(k, g, nullptr, nullptr, s);
  dense_factor_solve(d.L, d.npad, d.ld, g->Ldiag, d.x, done, sc, g->dd,
                     dense_launch_plan_no_tail(sc, h->knobs.dense, g->dd.flow_ok, g->dd.plan[1], h->knobs.cone.want),
                     s);
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(&bad_now, g->dd.bad_pivots, sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(g->dd.bad_pivots, &bad_keep, sizeof(int), hipMemcpyHostToDevice));
  g->hc = keep;  // the controller as it was
  if (push_ctrl(g)) return -1;
  HIP_TRY(hipStreamSynchronize(s));
  if (bad_now >= kFlowTimeout) return fail(what + ": a dataflow hand-off of the factorisation timed out");
  // ---- the batches; everything below is freed again on every return
  ScratchAllocs scratch(h);
  constexpr Mem R = Mem::Resident;
  const bool cand = c.entry_kind == kPgCovCand;
  const size_t ne = (size_t)c.n_entry;
  const int gpb = cov_batch_cols(d.npad, h->knobs.run) / kCovGroupCols;  // groups per batch
  const int bw = (int)std::min<size_t>(gpb, std::max<size_t>(1, groups.size())) * kCovGroupCols;
  int *d_trow_ptr = nullptr, *d_trow = nullptr;
  PgCovGroup *d_groups = nullptr;
  double *Zw = nullptr, *d_val = nullptr;
  GraphCovOut out{};
  g->cov_batches = 0;
  if (!groups.empty()) {
    std::vector<double> val;
    if (cand) k.pack_values(c.n_entry, c.Z, c.Omega, &val);
    if (h->upload(R, &d_trow_ptr, trow_ptr) || h->upload(R, &d_trow, trow) || h->upload(R, &d_groups, groups) ||
        h->dalloc(R, &Zw, (size_t)d.npad * bw) || h->dalloc(R, &out.pose, (size_t)n_pose_rows * WW) ||
        h->dalloc(R, &out.rel, ne * WW) || (c.cov_cross && h->dalloc(R, &out.cross, ne * WW)) ||
        (cand && (h->upload(R, &d_val, val) || h->dalloc(R, &out.d2, ne))) ||
        (cand && c.r && h->dalloc(R, &out.r, ne * W)) || (cand && c.innov && h->dalloc(R, &out.innov, ne * WW)))
      return -1;
    for (size_t g0 = 0; g0 < groups.size(); g0 += gpb) {  // fixed batch order
      const int ng = (int)std::min<size_t>(gpb, groups.size() - g0);
      k.cov_batch(d, g->Ldiag, g->nb, g->ncb, d.poses[keep.cur], d_trow_ptr, d_trow, d_groups + g0, ng, d_val, Zw, bw,
                  out, s);
      ++g->cov_batches;
    }
  }
  std::vector<double> hp, hrel, hcross, hd2, hr, hP;
  if (download(hp, out.pose, (size_t)n_pose_rows * WW, s) || download(hrel, out.rel, out.rel ? ne * WW : 0, s) ||
      download(hcross, out.cross, out.cross ? ne * WW : 0, s) || download(hd2, out.d2, out.d2 ? ne : 0, s) ||
      download(hr, out.r, out.r ? ne * W : 0, s) || download(hP, out.innov, out.innov ? ne * WW : 0, s))
    return -1;
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipGetLastError());
  for (int q = 0; q < c.n_pose_sel; ++q)
    std::memcpy(c.cov_pose + (size_t)q * WW, &hp[(size_t)slot_of_opt[g->lists.opt_of_pose[c.pose_sel[q]]] * WW],
                WW * sizeof(double));
  auto give = [](double *dst, const std::vector<double> &src) {
    if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(double));
  };
  if (!cand) give(c.cov_rel, hrel);
  give(c.cov_cross, hcross);
  give(c.d2, hd2);
  give(c.r, hr);
  give(c.innov, hP);
  if (dropped_pivots) *dropped_pivots = bad_now;
  return 0;
}

}  // namespace

// what was allocated on the handle since `mark` belongs to the graph from here on
void graph_adopt_allocs(GraphHost *g, size_t mark) {
  ba_handle *h = g->h;
  g->allocs.insert(g->allocs.end(), h->allocs.begin() + mark, h->allocs.end());
  h->allocs.resize(mark);
}

// the controller for a pass outside the LM loop: the accepted buffer stays
int graph_begin_pass(GraphHost *g) {
  g->hc.done = 0;
  g->hc.relin = 1;
  g->hc.lambda = 0.0;
  return push_ctrl(g);
}

int graph_create(const GraphSpec &k, GraphHost *g, ba_handle *h, int n_pose, const double *poses,
                 const uint8_t *pose_fixed, int64_t n_rel, const int32_t *rel_j, const int32_t *rel_k,
                 const double *Z, const double *Omega) {
  HIP_TRY(hipSetDevice(h->device));
  g->h = h;
  g->n_pose = n_pose;
  g->F = n_rel;
  if (pose_fixed)
    g->fixed.assign(pose_fixed, pose_fixed + n_pose);
  else
    g->fixed.assign((size_t)n_pose, 0);
  g->Z.assign(Z, Z + (size_t)k.pose_doubles * n_rel);
  g->Om.assign(Omega, Omega + (size_t)k.W * k.W * n_rel);
  pgraph_build_lists(n_pose, g->fixed.data(), n_rel, rel_j, rel_k, &g->lists);
  const size_t mark = h->allocs.size();
  const int rc = build_device(k, g, poses);
  graph_adopt_allocs(g, mark);
  if (rc) free_device(g);
  return rc;
}

void graph_destroy(GraphHost *g) {
  (void)hipSetDevice(g->h->device);
  (void)hipStreamSynchronize(g->h->stream);
  free_device(g);
}

int graph_update_values(const GraphSpec &k, GraphHost *g, const double *poses, const double *Z, const double *Omega) {
  ba_handle *h = g->h;
  std::string err;
  if (k.validate_values(g->n_pose, poses, g->F, Z, Omega, &err))
    return fail(std::string(k.abi) + "_update_values: " + err);
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (Z || Omega) {
    if (Z) g->Z.assign(Z, Z + (size_t)k.pose_doubles * g->F);
    if (Omega) g->Om.assign(Omega, Omega + (size_t)k.W * k.W * g->F);
    std::vector<double> val;
    k.pack_values(g->F, g->Z.data(), g->Om.data(), &val);
    HIP_TRY(hipMemcpy(g->val, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  if (poses) {
    const size_t bytes = (size_t)g->n_pose * k.pose_doubles * sizeof(double);
    HIP_TRY(hipMemcpy(g->d.poses[0], poses, bytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g->d.poses[1], poses, bytes, hipMemcpyHostToDevice));
    g->hc.cur = 0;
  }
  return 0;
}

int graph_set_robust(GraphHost *g, const int32_t *kind, const double *scale) {
  const size_t F = (size_t)g->F;
  std::vector<int32_t> k(F, 0);
  std::vector<double> c(F, 0.0);
  bool any = false;
  for (size_t f = 0; kind && f < F; ++f)
    if (kind[f] != 0) {
      k[f] = kind[f];
      c[f] = scale[f];
      any = true;
    }
  if (!any && !g->d_rkind) {  // never robust, and stays so: nothing to allocate
    g->robust = false;
    return 0;
  }
  ba_handle *h = g->h;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (ensure_robust_arrays(g)) return -1;
  HIP_TRY(hipMemcpy(g->d_rkind, k.data(), F * sizeof(int32_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(g->d_rscale, c.data(), F * sizeof(double), hipMemcpyHostToDevice));
  g->rkind.swap(k);
  g->rscale.swap(c);
  g->robust = any;
  return 0;
}

int graph_factor_weights(const GraphSpec &k, GraphHost *g, double *s, double *w) {
  ba_handle *h = g->h;
  HIP_TRY(hipSetDevice(h->device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (ensure_robust_arrays(g)) return -1;
  if (graph_begin_pass(g)) return -1;
  // one cost-only pass at the accepted poses; the report has arrays of its own, so that rb.s and
  // rb.w stay those of the records
  PgRobust rep = g->rb;
  rep.s = g->d_rep_s;
  rep.w = g->d_rep_w;
  k.lin_robust(g->d, rep, 3, h->stream);
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipGetLastError());
  const size_t bytes = (size_t)g->F * sizeof(double);
  if (s) HIP_TRY(hipMemcpy(s, g->d_rep_s, bytes, hipMemcpyDeviceToHost));
  if (w) HIP_TRY(hipMemcpy(w, g->d_rep_w, bytes, hipMemcpyDeviceToHost));
  return 0;
}

int graph_solve(const GraphSpec &k, GraphHost *g, const ba_options *opt, ba_iter_info *rows, int cap, int *n_iter,
                int *converged) {
  ba_handle *h = g->h;
  if (n_iter) *n_iter = 0;
  if (converged) *converged = 1;
  if (opt->max_num_iterations <= 0) return 0;
  HIP_TRY(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  const PgDev &d = g->d;
  PgCtrl &c = g->hc;
  const int cur = c.cur;
  std::memset(&c, 0, sizeof(c));
  c.cur = cur;
  c.lambda = (double)opt->initial_lambda;
  c.thr_step = (double)opt->threshold_step_size;
  c.thr_cost = (double)opt->threshold_cost_change;
  c.dec_ratio = (double)opt->decrease_ratio_lambda;
  c.inc_ratio = (double)opt->increase_ratio_lambda;
  c.max_iter = opt->max_num_iterations;
  c.gn = opt->gauss_newton ? 1 : 0;
  c.relin = 1;
  if (push_ctrl(g)) return -1;
  HIP_TRY(hipMemsetAsync(g->dd.bad_pivots, 0, sizeof(int), s));
  g_ktimer = h->timing ? &h->kt : nullptr;
  const int *done = done_flag(g);
  HIP_TRY(hipEventRecord(g->e0, s));
  for (int it = 0; it < opt->max_num_iterations; ++it) {
    lin(k, g, 0, s);
    launch_dense_init(d.L, d.ld, g->col_x, g->zt_I, g->zt_J, g->n_zt, g->nb, done, s);
    assemble(k, g, nullptr, nullptr, s);
    dense_factor_solve(d.L, d.npad, d.ld, g->Ldiag, d.x, done, g->sched, g->dd, g->dd.plan[g->dd.flow_ok], s);
    k.trial(d, s);
    lin(k, g, 1, s);
    launch_pg_control(d, 0, s);  // (knows nothing of a pose's width: the one controller of both kinds)
  }
  HIP_TRY(hipEventRecord(g->e1, s));
  g_ktimer = nullptr;
  if (pull_ctrl(g)) return -1;
  if (h->timing) h->kt.collect();
  HIP_TRY(hipGetLastError());
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, g->e0, g->e1);
  g->last_ms = ms;
  int bad = 0;
  HIP_TRY(hipMemcpy(&bad, g->dd.bad_pivots, sizeof(int), hipMemcpyDeviceToHost));
  if (bad >= kFlowTimeout) return fail(std::string(k.abi) + "_solve: a dataflow hand-off timed out");
  g->bad_pivots = bad;
  static_assert(sizeof(DevIterRec) == sizeof(ba_iter_info), "row layout");
  const int n = std::min(std::min(c.iter, cap), d.log_cap);
  if (n > 0) HIP_TRY(hipMemcpy(rows, d.log, (size_t)n * sizeof(ba_iter_info), hipMemcpyDeviceToHost));
  if (n_iter) *n_iter = c.iter;
  if (converged) *converged = c.converged;
  return 0;
}

int graph_get_poses(const GraphSpec &k, GraphHost *g, double *poses) {
  HIP_TRY(hipSetDevice(g->h->device));
  HIP_TRY(hipStreamSynchronize(g->h->stream));
  HIP_TRY(hipMemcpy(poses, g->d.poses[g->hc.cur], (size_t)g->n_pose * k.pose_doubles * sizeof(double),
                    hipMemcpyDeviceToHost));
  return 0;
}

int graph_cost(const GraphSpec &k, GraphHost *g, double *chi2) {
  HIP_TRY(hipSetDevice(g->h->device));
  if (graph_begin_pass(g)) return -1;
  lin(k, g, 2, g->h->stream);
  launch_pg_control(g->d, 1, g->h->stream);
  if (pull_ctrl(g)) return -1;
  HIP_TRY(hipGetLastError());
  *chi2 = g->hc.aux;
  return 0;
}

int graph_get_system(const GraphSpec &k, GraphHost *g, double *H, double *gWN) {
  ba_handle *h = g->h;
  HIP_TRY(hipSetDevice(h->device));
  const size_t nW = (size_t)k.W * g->d.N;
  double *dH = nullptr, *dg = nullptr;
  HIP_TRY(hipMalloc((void **)&dH, nW * nW * sizeof(double)));
  if (hipMalloc((void **)&dg, nW * sizeof(double)) != hipSuccess) {
    (void)hipFree(dH);
    return fail(std::string(k.abi) + "_get_system: hipMalloc");
  }
  int rc = 0;
  if (hipMemsetAsync(dH, 0, nW * nW * sizeof(double), h->stream) != hipSuccess || graph_begin_pass(g)) rc = -1;
  if (!rc) {
    lin(k, g, 0, h->stream);
    assemble(k, g, dH, dg, h->stream);
    if (hipStreamSynchronize(h->stream) != hipSuccess || hipGetLastError() != hipSuccess ||
        (H && hipMemcpy(H, dH, nW * nW * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) ||
        (gWN && hipMemcpy(gWN, dg, nW * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
      rc = fail(std::string(k.abi) + "_get_system: device error");
  }
  (void)hipFree(dH);
  (void)hipFree(dg);
  return rc;
}

int graph_covariance(const GraphSpec &k, GraphHost *g, int n_pose_sel, const int32_t *pose_sel, double *cov_pose,
                     int64_t n_pair, const int32_t *pair_j, const int32_t *pair_k, double *cov_cross,
                     double *cov_rel, int64_t *dropped_pivots) {
  GraphCovCall c;
  c.n_pose_sel = n_pose_sel;
  c.pose_sel = pose_sel;
  c.cov_pose = cov_pose;
  c.n_entry = n_pair;
  c.entry_j = pair_j;
  c.entry_k = pair_k;
  c.cov_cross = n_pair > 0 ? cov_cross : nullptr;
  c.cov_rel = cov_rel;
  return graph_cov_run(k, g, std::string(k.abi) + "_covariance", c, dropped_pivots);
}

int graph_gate(const GraphSpec &k, GraphHost *g, int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k,
               const double *Z, const double *Omega, double *d2, double *r, double *innov, int64_t *dropped_pivots) {
  GraphCovCall c;
  c.n_entry = n_cand;
  c.entry_kind = kPgCovCand;
  c.entry_j = cand_j;
  c.entry_k = cand_k;
  c.Z = Z;
  c.Omega = Omega;
  c.d2 = d2;
  c.r = n_cand > 0 ? r : nullptr;
  c.innov = n_cand > 0 ? innov : nullptr;
  return graph_cov_run(k, g, std::string(k.abi) + "_gate", c, dropped_pivots);
}

void graph_cov_info(const GraphHost *g, int64_t out4[4]) {
  const int bw = cov_batch_cols(g->d.npad, g->h->knobs.run);
  out4[0] = bw;
  out4[1] = kCovGroupCols;
  out4[2] = g->cov_batches;
  out4[3] = (int64_t)g->d.npad * bw * (int64_t)sizeof(double);
}

void graph_info(const GraphHost *g, int64_t out8[8]) {
  out8[0] = g->d.N;
  out8[1] = g->F;
  out8[2] = g->d.nblk;
  out8[3] = g->nb;
  out8[4] = g->ncb;
  out8[5] = g->sched.nlev;
  out8[6] = (int64_t)g->image_bytes;
  out8[7] = g->bad_pivots;
}

double graph_last_ms(const GraphHost *g) { return g->last_ms; }

}  // namespace ba
