// ba_device.h — device-side structures and launcher prototypes shared by the
// HIP translation units (internal; the public boundary is include/ba_hip.h).
#ifndef BA_DEVICE_H_
#define BA_DEVICE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

#include "ba_dense_sched.h"

namespace ba {

// LM controller state, resident in device memory so that a whole batch of
// iterations can be enqueued without host round trips.  Mirrors the locals of
// reference core/full_bundle_adjustment_solver.cpp:705-1008.
struct DevCtrl {
  double lambda;
  double prev_cost;
  double huber;
  double thr_step;
  double thr_cost;
  double dec_ratio;
  double inc_ratio;
  unsigned long long t_last;  // wall_clock64 stamp of the previous iteration
  int cur;        // which parameter buffer holds the accepted parameters
  int done;       // set once converged / max_iter reached: kernels no-op
  int iter;       // iterations completed
  int converged;
  int max_iter;
  int gn;         // 1: plain Gauss-Newton (always accept, lambda fixed)
  int lcur;       // which block buffer holds the linearisation at the accepted parameters
  // Parameter / block buffers of the TRIAL point of the iteration in flight,
  // written by k_pose_update before the trial-point linearisation starts.  The
  // pose side of that linearisation runs on the side stream and may execute after
  // the control step has flipped cur / lcur: it must not derive "trial" from them.
  int tcur, tlcur;
  int pad_;
};

struct DevIterRec {  // layout-identical to ba_iter_info
  double cost, cost_change, average_reprojection_error, abs_gradient, abs_step,
      damping_term, iter_time_ms;
  int iteration_status, pad_;
  double rho, model_change, trial_cost;
};

// All device pointers of one problem shard.
// B_ji = w Q^T R (6x3, reference :826) has the structure [K ; [X_ij]x K] with
// K = w G^T R (3x3, = rows 0..2 of B_ji bit for bit) and X_ij the point in the
// pose frame: Q = [G, G(-[X_ij]x)].  HBM holds the 12 doubles {K row-major,
// X_ij} per pair (96 B instead of 144); consumers rebuild rows 3..5 as
// X_ij x (column of K), or use B^T x = K^T (x_t + x_r x X_ij) directly.
constexpr int kWStride = 12;
// Pairs of covisibility groups that k_lin_grp linearises (DevProblem::pair_slim) keep less:
// {G (2x3 row-major), w, 0} of the pair's last writer, 8 doubles.  K = G^T (w G R_jw) and
// X_ij = R_jw X_i + t_jw are rebuilt by the readers (pair_from_G, ba_device_fn.h), for which
// the pose is a lane constant and the point a per-landmark load.  The grouped pairs are the
// first P_slim pairs; slim record p lies at double p * kWSlim of the same array W[], i.e.
// inside the grouped pairs' own 96-byte range, and pair p >= P_slim stays at p * kWStride.
constexpr int kWSlim = 8;
// "From the observation" (DevProblem::pair_obs): a slim handle whose groups are all 32 wide
// (at most kPairObsPoses free poses) and none of them masked keeps NO record of the grouped
// pairs in the iteration.  {G, w} is a function of the last writer's observation (16 bytes),
// its camera, the pose and the point at the linearisation point (pair_G_from_obs,
// ba_device_fn.h): k_lin_grp writes nothing, k_schur_grp<2> and the group role of
// k_backsub_update fetch that observation and rebuild {G, w}, then {K, X_ij}.  Readers off the
// hot path (ba_get_pairs, ba_covariance) first have k_pair_records fill the slim records of
// buffer ctrl->lcur and then run as with the slim form.  Per group piece (LinDesc) and per
// k_schur_grp workgroup (GrpDesc) one PairObs: obs(il, last slot of pose jj) = o0 + no * il +
// (sc[jj] & 0xff), through camera sc[jj] >> 8.
constexpr int kPairObsPoses = 5;
struct PairObs {
  int64_t o0;
  int32_t no;
  int32_t sc[kPairObsPoses];
};

struct DevProblem {
  // sizes
  int n_cam, n_pose, N, n_pt, M, M_global;
  int64_t n_obs, n_obs_opt, n_obs_global, P, n_pobs, T, B;
  int n_achunk, n_tchunk;
  // parameters: two buffers each (accepted / trial), selected by ctrl->cur
  double *cams;      // n_cam*16: fx fy cx cy R9 t3
  double *poses[2];  // n_pose*12
  double *pts[2];    // n_pt*3
  // landmark-major observations
  int4 *obs_idx;
  double2 *obs_uv;
  int64_t *lm_obs_ptr;
  int64_t *lm_pair_ptr;
  int32_t *pair_pose;
  int32_t *pair_lm;
  // pose-major observations
  int2 *pobs_idx;   // {camera, point}
  int2 *obs_cp;     // n_obs {camera | pose << 16, point} for k_cost, or null (>= 65536 cameras / poses)
  double2 *pobs_uv;
  int32_t *achunk_pose;
  int64_t *achunk_begin, *achunk_end;
  int32_t *pose_achunk_ptr;
  // pose-major pairs
  // Schur structure
  int32_t *sblk_j, *sblk_k;
  int32_t *diag_blk;
  int64_t *tri_p, *tri_q;
  int32_t *tchunk_blk;
  int64_t *tchunk_begin, *tchunk_end;
  int32_t *sblk_tchunk_ptr;
  // Schur super-runs (landmark-major, register-resident slot accumulators)
  int n_sup, n_slot;
  struct SupDesc {
    int32_t s0, ns, chunk_begin, chunk_end;
  };
  struct ChunkDesc {
    int64_t p0, tb, sp;
    int32_t l0, nl, np, nt;
  };
  // covisibility groups (k_schur_grp): layout-identical to Plan::GrpDesc
  struct GrpDesc {
    int64_t p0;
    int32_t l0, nl, d, s0;
    int32_t pose[20];
    int32_t pad_[6];
  };
  struct LinDesc {  // one k_lin_grp workgroup: layout-identical to Plan::LinDesc
    int64_t p0, o0;
    int32_t l0, nl, d, no;
    int32_t pat0;
    int32_t apart0, cost_idx;
    int32_t pad_;
  };
  LinDesc *lin_desc;
  int n_lin_desc;
  int n_lin_plain;  // pieces [0, n_lin_plain): exact groups; behind them: masked (superset) groups
  GrpDesc *grp32, *grp64, *grp128;  // pose sets of <= 5 / 6..10 / 11..20 poses
  int n_grp32, n_grp64, n_grp128;
  // k_lin_grp (groups linearised landmark and pose side in one pass): per pattern
  // slot {pose, camera | jj << 16 | optimisable << 29 | last writer << 30}
  int2 *grp_pat;
  double *Apart2;            // n_apart2 * 27 pose-side partial sums of the group pieces
  double *lin_dump;          // kLinDump doubles: target of k_lin_grp's lanes with nothing to store
  int32_t *pose_gpart_ptr, *pose_gpart;  // rows of Apart2 per pose
  int lin_chunk0;            // k_lin_landmarks starts at this chunk (the chunks before are k_lin_grp's)
  int n_lin_cost;            // entries of lin_cost_part: n_bchunk + k_lin_grp pieces
  int n_bs_grp;              // group-role workgroups of k_backsub_update (= n_lin_desc, or 0)
  int n_lm_part;             // entries of lm_part: n_bs_grp + chunk workgroups behind lin_chunk0
  int pair_slim;             // 1: the pairs [0, P_slim) are kept as kWSlim records (see kWSlim)
  int64_t P_slim;            // pairs of the grouped landmarks when pair_slim, else 0
  int pair_obs;              // 1: the iteration keeps no record of the pairs [0, P_slim) (see PairObs)
  PairObs *lin_obs, *grp_obs;  // when pair_obs: per lin_desc piece / per grp32 workgroup
  SupDesc *sup_desc;
  uint32_t *sup_lane;  // n_sup*256: lane -> (slot, half, position, lanes per half) of k_schur_lds
  ChunkDesc *chunk_desc;
  uint16_t *chunk_sp;
  uint32_t *ltri;
  int64_t *blk_contrib_ptr;
  int32_t *contrib_slot;
  // the same per block as ONE 64-byte record (k_schur_final reaches its slot partials
  // after one dependent load): {j, k, first contribution, #contributions, first triple
  // chunk, #triple chunks, 0, 0, first eight slots}
  int32_t *blk_desc;
  double *spart2;  // n_slot*kSlotStride slot partial sums (36 of S + 6 of rhs)
  // Linearisation blocks: TWO buffers each, selected by ctrl->lcur.  Every LM
  // iteration linearises at its TRIAL point into the other buffer (the trial cost
  // is a by-product of that pass: no separate cost kernel); accepting the step
  // flips lcur together with cur, rejecting it keeps the old blocks, which are
  // still the linearisation at the accepted point (reference :943-953 only
  // changes lambda then).  The blocks are stored UNDAMPED; the (1 + lambda)
  // scaling of the diagonals (reference :833-852) is applied where they are read.
  double *Cu[2];   // M*6   C_i upper (00 01 02 11 12 22), undamped
  double *b[2];    // M*3
  double *W[2];    // P*kWStride  compact B_ji (see kWStride); its first P_slim pairs as kWSlim records when pair_slim
  double *A[2];    // N*36  full (mirrored), undamped
  double *a[2];    // N*6
  double *Cinv;    // M*6   inverse of the damped C_i (k_damp_invert, after the control step)
  double *Cd;      // M*6   damped C_i: written only for the readers (ba_get_C)
  double *Apart;   // n_achunk*27
  double *spart;   // n_tchunk*kSlotStride
  double *x;       // 6N
  double *y;       // M*3
  // scalar reductions
  double *cost_part;   // kCostGrid (k_cost: stage API, observations of fixed landmarks)
  double *lin_cost_part;  // n_bchunk: sum of residual norms per k_lin_landmarks workgroup
  int64_t n_obs_lm;    // observations of optimisable landmarks = the first n_obs_lm of the
                       // landmark-major list (k_lin_landmarks sees exactly these)
  double *lm_part;     // n_lm_part*2 : model (landmark side), sum |y| per landmark workgroup of k_backsub_update
  double *pose_part;   // [0..1] totals, then kPoseGrid*2 block partials:
                       // model (pose side), sum |x|
  double *scal;        // exchange buffer 1: [0] cost [1] model est [2] sum|y|
  // controller
  DevCtrl *ctrl;
  DevIterRec *log;
  int log_cap;
  // packed reduced system (exchange buffer 0): B*36 block entries, then 6N rhs
  double *Spk;
  // dense reduced system: column-major lower, ld rows (rhs rides as row npad)
  double *L;
  int npad, ld;
  double *Ldiag;   // (npad/nb) * dense_ws_per_block(nb) (diagonal factors + inverses)
  int nb;          // tile order of the reduced system (32 or 64)
  int *pose_col;   // N: first dense column of optimised pose j
  int *col_x;      // npad: dense column -> 6*pose + r, or -1 (padding)
  int32_t *bchunk_lm;  // n_bchunk+1 landmark ranges (backsub)
  // the same chunks as one 32-byte record each, so that a workgroup knows its
  // landmark / pair / observation ranges after ONE dependent load
  struct LmChunk {
    int64_t pb, ob;           // first pair, first (landmark-major) observation
    int32_t l0, nl, np, no;   // first landmark, #landmarks, #pairs, #observations
  };
  LmChunk *lm_chunk;   // n_bchunk
  int n_bchunk;
  int *zt_I, *zt_J;  // tiles of L that are (re)initialised every iteration
  int n_zt;
};

constexpr int kLinDump = 64 * 4 * 4;
// added to DenseDev::bad_pivots by a dataflow sweep whose bounded poll gave up
constexpr int kFlowTimeout = 1 << 20;
constexpr int kBsChunks = 4;     // chunks per chunk-role workgroup of k_backsub_update
constexpr int kCostGrid = 1792;  // 7 waves/SIMD resident on 256 CUs
constexpr int kLmGrid = 1024;
constexpr int kPoseGrid = 16;
constexpr int kGdFixGrid = 1024;     // k_gd_points workgroups for the observations of fixed landmarks
constexpr int kGdChunk = 512;        // observations per k_gd_poses wave (one pose's list is cut into chunks)
constexpr int kSlotStride = 42;  // 6x6 block of B Cinv B^T + 6 of B Cinv b
// dense workspace per 64-column block: L11 (64x64) + four 16x16 tile inverses

// ---- optional per-kernel device timing (hipEvents around every launch) ----
// Enabled by ba_enable_stage_timing: bench.py uses it to measure the average
// launch duration of each kernel live, on the stream the kernels run on.
enum KernelId {
  K_COST = 0, K_LIN_LANDMARKS, K_LIN_POSES, K_POSE_FINALIZE, K_DENSE_INIT,
  K_SCHUR_LDS, K_SCHUR_PARTIAL, K_SCHUR_FINAL, K_SCATTER,
  K_CHOL_DIAG, K_CHOL_TRSM, K_CHOL_UPDATE, K_CHOL_BACK, K_CHOL_DIAG_TRSM, K_CHOL_TAIL, K_BACKSUB_UPDATE,
  K_POSE_UPDATE, K_SCALARS, K_CONTROL, K_DAMP_INVERT, K_SCHUR_GRP, K_LIN_GRP,
  K_REL_LIN, K_REL_GATHER, K_REL_OFFDIAG,
  K_S3_LIN, K_S3_ASSEMBLE, K_S3_TRIAL, K_S3_LIN_ROBUST, K_S3_ASSEMBLE_ROBUST,
  K_PG_LIN_ROBUST, K_PG_ASSEMBLE_ROBUST,
  K_PG_LIN, K_PG_ASSEMBLE, K_PG_TRIAL, K_PG_CONTROL, K_COUNT
};
struct KernelTimer {
  bool on = false;
  std::vector<hipEvent_t> pool;          // grows on demand
  std::vector<int> ids;                  // kernel id of span k (events 2k,2k+1)
  double ms[K_COUNT] = {0};
  long calls[K_COUNT] = {0};
  void begin(int id, hipStream_t s);
  void end(hipStream_t s);
  void collect();                        // after a stream sync
  void reset();
};
extern thread_local KernelTimer *g_ktimer;
// launch a kernel, bracketed by events when a timer is installed
#define BA_LAUNCH(id, kernel, grid, block, stream, ...)                     \
  do {                                                                      \
    if (::ba::g_ktimer && ::ba::g_ktimer->on) ::ba::g_ktimer->begin(id, stream); \
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);        \
    if (::ba::g_ktimer && ::ba::g_ktimer->on) ::ba::g_ktimer->end(stream);  \
  } while (0)

// Pins a wave-uniform 32-bit value: everything it depends on (typically a
// scalar load) has to be issued AND complete before this point, and the
// compiler cannot sink those loads below a later branch.  Used to request a
// workgroup's record together with the control word instead of one after the
// other (`if (ctrl->done) return;` first costs a full scalar-load latency).
#define BA_KEEP_S(x) asm volatile("" ::"s"(x))

// ---- launchers (ba_kernels.hip) ----
// sel: 0 = accepted parameters (block buffer lcur), 1 = trial parameters (the
// other block buffer)
// k_cost over the observations [begin, n_obs) of the landmark-major list
void launch_cost(const DevProblem &d, int sel, int64_t begin, hipStream_t s);
// pose side (A_j, a_j) and landmark side (C_i, b_i, W_ji + the cost partials) of
// the linearisation at the `sel` parameters
void launch_lin_poses(const DevProblem &d, int sel, hipStream_t s);
void launch_lin_landmarks(const DevProblem &d, int sel, hipStream_t s);
void launch_damp_invert(const DevProblem &d, hipStream_t s);
// pair_obs handles: the slim records of the grouped pairs of buffer ctrl->lcur, from the observations
void launch_pair_records(const DevProblem &d, hipStream_t s);
// dense_init + Schur accumulation + finalisation; direct: single GPU, S and rhs are
// also placed in the dense matrix (no k_scatter); with_init: also reset the factor tiles
void launch_schur(const DevProblem &d, bool direct, bool with_init, hipStream_t s);
void launch_schur_accumulate(const DevProblem &d, hipStream_t s);
void launch_schur_final(const DevProblem &d, bool direct, hipStream_t s);
void launch_backsub_update(const DevProblem &d, hipStream_t s, bool zero_tiles = false);
void launch_scatter(const DevProblem &d, hipStream_t s);
// cost_src: 0 = the k_cost partials only (stage API), 1 = the k_lin_landmarks
// partials (+ the k_cost partials of fixed-landmark observations, if any)
void launch_scalars_cost_only(const DevProblem &d, int cost_src, hipStream_t s);
void launch_scalars(const DevProblem &d, int cost_src, hipStream_t s);
void launch_scalars_and_control(const DevProblem &d, int cost_src, hipStream_t s,
                                int finalize_sel = -1);  // single GPU; finalize_sel >= 0: + k_pose_finalize workgroups
void launch_control(const DevProblem &d, hipStream_t s);
void launch_init_ctrl_cost(const DevProblem &d, hipStream_t s);

// ---- relative-pose factors of the handle path (ba_rel.hip, ba_set_relative) ----
// The factor arrays have a record of their own, an argument of the k_rel_* kernels only:
// DevProblem, which every hot kernel takes by value, does not grow.  F = 0: no factors, and
// nothing of this is launched.
constexpr int kRelFpb = 64;  // factors per k_rel_lin workgroup
constexpr int kRelScr = 126;  // scratch record of one factor, handle and batch paths (its layout: ba_rel_fn.h)
struct RelDev {
  int F;                  // factors
  int nblk;               // coupled blocks of S (two optimisable poses)
  int n_part;             // workgroups of k_rel_lin = cdiv(F, kRelFpb)
  int pad_;
  const int4 *jk;         // per factor: {pose j, pose k (internal), optimised index of j or -1, of k or -1}
  const double *val;      // per factor: Z (12), Omega (36, mirrored by the host)
  const int32_t *pptr, *plist;  // per optimised pose, input order: factor << 1 | (1: it is the factor's k)
  const int32_t *blk;           // per coupled block: its id in sblk_j / sblk_k
  const int32_t *bptr, *blist;  // per coupled block, input order: factor << 1 | (1: S_jk lies transposed)
  double *scr[2];         // kRelScr doubles per factor, one per block buffer
  double *part;           // 2 per k_rel_lin workgroup: sum of the factors' norms, cross term of the model
};
// mode bit 0: linearise at the `sel` poses into the scratch of that block buffer; bit 1: the
// model's cross term from the accepted point's Omega Ad (scratch lcur) and x.  Always: the
// factors' norms at the `sel` poses.  Both sums go to r.part.
void launch_rel_lin(const DevProblem &d, const RelDev &r, int sel, int mode, hipStream_t s);
// flags bit 0: add the factors' diagonal blocks and gradients to A_j, a_j of the `sel` block
// buffer; bit 1: scal[0] += the norms; bit 2: scal[1] += the cross term (workgroup 0)
void launch_rel_gather(const DevProblem &d, const RelDev &r, int sel, int flags, hipStream_t s);
// S_jk += -Omega Ad of every coupled block into Spk (direct: and into the dense image)
void launch_rel_offdiag(const DevProblem &d, const RelDev &r, bool direct, hipStream_t s);

// ---- pose-graph optimisation (ba_graph_kernels.hip, ba_pgraph_*) ----
// LM over relative-pose factors alone: chi2 = sum_f r_f^T Omega_f r_f, no landmark in the
// problem.  The controller lives on the device, as DevCtrl does for the handle path, so that
// max_num_iterations iterations are enqueued without a host round trip; `done` is the control
// word that dense_factor_solve and every k_pg_* kernel test first.  The host side is the graph
// driver of ba_graph.hip: it holds a PgDev and a PgCtrl per graph and reaches the launchers below
// through the graph kind's GraphSpec (ba_graph.h), the SE(3) kind's in ba_pgraph.hip.
struct PgCtrl {
  double lambda;
  double chi2;      // chi-square at the accepted poses
  double thr_step, thr_cost, dec_ratio, inc_ratio;
  double aux;       // k_pg_control, mode 1: chi-square of the last cost-only pass
  unsigned long long t_last;
  int cur;          // which pose buffer holds the accepted poses
  int done;
  int iter, converged, max_iter, gn;
  int relin;        // the records belong to another point than the accepted one
  int pad_;
};
constexpr int kPgFpb = 64;   // factors per k_pg_lin workgroup
constexpr int kPgRec = 84;   // record of one factor: Omega r (6), Ad^T Omega r (6), Omega Ad (36), Ad^T Omega Ad (36)
constexpr int kPgOr = 0, kPgGk = 6, kPgOA = 12, kPgBk = 48;
struct PgDev {
  int n_pose, N, F, nblk;
  int n_part;             // workgroups of k_pg_lin = cdiv(F, kPgFpb)
  int n_tpart;            // workgroups of k_pg_trial = cdiv(N, 256)
  int npad, ld;           // the dense image: npad columns of ld rows, g in row npad
  double *poses[2];       // 12 per pose (user order); a fixed pose has the same bits in both
  const int4 *jk;         // per factor: {pose j, pose k, optimisable index of j or -1, of k or -1}
  const double *val;      // per factor: Z (12), Omega (36, mirrored by the host)
  const int32_t *pptr, *plist;  // per optimisable pose, input order: factor << 1 | (1: it is the factor's k)
  const int2 *blk;              // per coupled block: optimisable poses {hi, lo}, hi > lo
  const int32_t *bptr, *blist;  // per coupled block, input order: factor << 1 | (1: H_jk lies transposed)
  const int32_t *opt_pose;      // per optimisable pose: its pose
  const int *pose_col;          // per optimisable pose: its first column of the image
  double *rec;            // kPgRec doubles per factor
  double *dH, *g;         // 6N each: diag(H) and g of the last assembly
  double *x;              // 6N (+ 64)
  double *part[2];        // n_part each: chi-square partials of the linearisation / of a cost-only pass
  double *tpart;          // 2 n_tpart: partials of sum |x_j| and of pred
  double *L;
  PgCtrl *ctrl;
  DevIterRec *log;
  int log_cap;
};
// Robust kernels of the factors (ba_pgraph_set_robust): a record of their own, an
// argument of the robust instantiations only, so that PgDev and the plain kernels stay as they are.
struct PgRobust {
  const int32_t *kind;    // per factor: 0 none, 1 Huber, 2 Cauchy, 3 Geman-McClure
  const double *scale;    // per factor: c (a Mahalanobis distance); unread where kind is 0
  double *s, *w;          // per factor: s = r^T Omega r and w = rho'(s) of the pass that wrote them
};
// The launchers of the graph kernels (ba_graph_kernels.hip), one template per kernel, instantiated
// there for the two groups of ba_graph_fn.h; W is the group's tangent width.
struct Se3Graph;
struct Sim3Graph;
// cost_only = 0: linearise at the accepted poses (records + part[0]; skipped while !ctrl->relin);
// 1: chi-square partials at the trial poses -> part[1]; 2: at the accepted poses -> part[1]
template <class G>
void launch_graph_lin(const PgDev &p, int cost_only, hipStream_t s);
// the same with sum rho(s) for chi-square and w Omega for Omega; rb.s and rb.w are written by
// cost_only = 0 (they belong to the records) and by cost_only = 3 (= 2 plus the report)
template <class G>
void launch_graph_lin_robust(const PgDev &p, const PgRobust &rb, int cost_only, hipStream_t s);
// H + lambda diag(H) and g into the image (Hout == nullptr), or the undamped H (W N x W N,
// both triangles) and g into Hout / gout
template <class G>
void launch_graph_assemble(const PgDev &p, double *Hout, double *gout, hipStream_t s);
template <class G>
void launch_graph_assemble_robust(const PgDev &p, const PgRobust &rb, double *Hout, double *gout, hipStream_t s);
template <class G>
void launch_graph_trial(const PgDev &p, hipStream_t s);
// mode 0: the trust-region step of one iteration; 1: ctrl->aux = sum of part[1]
void launch_pg_control(const PgDev &p, int mode, hipStream_t s);

// ---- Sim(3) pose graph (ba_graph_kernels.hip, ba_sim3_*) ----
// The 7-DoF graph has the pose graph's device record and controller: PgDev with 13 doubles per
// pose (R, t, s), 62 per factor in val (Z 13, Omega 49 mirrored), kS3Rec per factor in rec, and
// 7N where PgDev says 6N.  k_pg_control knows nothing of a pose's width and runs as it is, and so
// does the host driver (ba_graph.hip): the widths and the launchers above at Sim3Graph are the
// Sim(3) kind's GraphSpec in ba_sim3.hip.
constexpr int kS3Fpb = 32;   // factors per k_s3_lin workgroup
constexpr int kS3Rec = 112;  // record of one factor: Omega r (7), Ad^T Omega r (7), Omega Ad (49), Ad^T Omega Ad (49)
constexpr int kS3Or = 0, kS3Gk = 7, kS3OA = 14, kS3Bk = 63;
// launch_graph_lin<Sim3Graph> with rep != nullptr: also s_f = r^T Omega r per factor into rep
// (ba_sim3_factor_report)
void launch_s3_lin(const PgDev &p, int cost_only, double *rep, hipStream_t s);

// ---- gradient descent (FullBundleAdjustmentSolverRefactor::SolveByGradientDescent) ----
// Device state of the first-order loop (ba_gd_*), allocated on the first GD call after
// ba_finalize.  It reads the problem's parameter buffer ctrl->cur and updates it in
// place; the LM blocks, lists and schedules are not touched.
struct GdDev {
  // pose-major index of EVERY real observation of an optimisable pose (the LM
  // pose-major list leaves out the covisibility groups; padded slots are not in it),
  // landmark-major order inside a pose, cut into chunks of one pose each
  int2 *pobs;       // {camera, point}
  double2 *puv;
  int32_t *chunk_pose;
  int64_t *chunk_begin, *chunk_end;
  int32_t *pose_chunk_ptr;  // N+1
  int n_chunk;
  double *ppart;      // n_chunk*6: sum of Q^T w r per chunk
  double *a;          // N*6: a_j = -sum Q^T w r (unclipped)
  double *b;          // M*3: b_i = -sum R^T w r (unclipped)
  double *cost_part;  // n_cost_part: sum of ||r|| per k_gd_points workgroup
  int n_cost_part;    // n_bchunk landmark chunks, then n_fix_blk blocks of fixed-landmark observations
  int n_fix_blk;
  double *step_part;  // n_upd_blk*2: {sum ||a_j||, sum ||b_i||} of the clipped blocks per workgroup
  int n_upd_pose_blk, n_upd_blk;
};
// pass over the observations at the current parameters: cost partials, b_i (landmark
// chunks) and the pose chunk partials
void launch_gd_pass(const DevProblem &d, const GdDev &g, hipStream_t s);
// mode 0: initial cost (previous_cost of reference :1158); 1: log row, stop rule.
// Both also sum the pose chunk partials into a_j.
void launch_gd_control(const DevProblem &d, const GdDev &g, int mode, hipStream_t s);
// clip, T_jw <- exp(a_j) T_jw, X_i <- X_i + b_i, step-norm partials
void launch_gd_update(const DevProblem &d, const GdDev &g, hipStream_t s);

// ---- dense solver (ba_dense.hip) ----
// Factor the npad x npad lower matrix in d.L (with the rhs carried as row
// `npad`) and write x (6N entries, pose order).
// Device copies of the static work lists of the level-scheduled Cholesky
// (host side: DenseSchedule in ba_dense_sched.h).
struct DenseDev {
  int *row_ptr = nullptr, *rows = nullptr;       // per position
  int *item_t = nullptr, *item_I = nullptr;      // TRSM items
  int *tgt_I = nullptr, *tgt_J = nullptr;        // update targets
  int *tgt_src_ptr = nullptr, *src_t = nullptr;  // their source panels
  int *tgt_desc = nullptr, *back_desc = nullptr; // 8-int inline records
  int *row_desc = nullptr;                       // 16-int records: row tiles of a position
  int *col_x = nullptr;   // npad: column -> index into x (6*pose + r) or -1
  double *xc = nullptr;   // npad: solution in column order
  int *bad_pivots = nullptr;  // device counter of non-positive pivots (or null)
  // dataflow backward sweep (k_chol_back_flow): tile positions top level first, one flag
  // per tile, the ticket counter; flow_gen = generation number of the next solve (host)
  int *flow_order = nullptr, *flow_flags = nullptr, *flow_ticket = nullptr;
  // forward sweep, one dataflow launch per level (k_chol_level_flow): one flag per tile
  // ("factorised, row tiles solved"), the ticket counter
  int *fwd_flags = nullptr, *fwd_ticket = nullptr;
  // forward sweep of the three-kernel path as one dataflow launch with lookahead (k_chol_dag):
  // per update target the updates of earlier levels on its column, per position all updates
  // on its column, the columns' counters of finished updates (n_fwd_cnt of them; also
  // k_chol_look's), items {kind, index}, TRSM items per position, "tile factorised" flags,
  // per-column counters of finished TRSM items (shares fwd_flags / fwd_ticket)
  int *upd_pre = nullptr, *col_need = nullptr, *fwd_cnt = nullptr;
  int n_fwd_cnt = 0;
  int *dag_items = nullptr, *dag_ntrsm = nullptr, *dag_dflags = nullptr, *dag_tcnt = nullptr;
  int *look_need = nullptr;  // k_chol_look: per position, the previous level's targets in its column
  int *cone_rec = nullptr;   // k_chol_back_cone: the step records of every leaf (DenseCone::rec), if plan[1].back_cone
  mutable int flow_gen = 0;
  // what dense_factor_solve launches (ba_dense_sched.h), as decided when the schedule was
  // uploaded: plan[flow_ok]
  DenseLaunchPlan plan[2];
  bool flow_ok = true;  // false while a hipGraph is captured / replayed (the generation is a kernel argument)
};
void launch_dense_solve(const DevProblem &d, const DenseSchedule &sc,
                        const DenseDev &dd, hipStream_t s);
// stand-alone form for ba_dense_spd_solve (x receives n_x entries via col_x) and ba_covariance
void dense_factor_solve(double *L, int npad, int ld, double *Ldiag, double *x,
                        const int *done_flag, const DenseSchedule &sc,
                        const DenseDev &dd, const DenseLaunchPlan &plan, hipStream_t s);
void launch_dense_init(double *L, int ld, const int *col_x, const int *zt_I,
                       const int *zt_J, int n_zt, int nb, const int *done_flag,
                       hipStream_t s);

// ---- covariance blocks (ba_cov.hip) ----
// One wave of k_cov_solve owns kCovGroupCols right-hand sides: two poses (kind 0, six
// identity columns each) or five landmarks (kind 1, three columns each).  item = optimised
// pose / internal landmark index, slot = row of the output array, t0 = tile position of
// the first non-zero row of the group's right-hand sides (ncb: none).
constexpr int kCovGroupCols = 16;
struct CovGroup {
  int32_t t0, kind, n, pad_;
  int32_t item[5], slot[5];
  int32_t pad2_[2];
};
static_assert(sizeof(CovGroup) == 64, "CovGroup is one 64-byte record");
// One column batch on the factored image of d (d.L, d.Ldiag, lambda = 0 blocks in buffer
// lcur, linearised at the poses and points of buffer cur, d.Cinv): zero the workspace Zw (d.npad x bw doubles, row-major, bw = 16 ng), place
// the right-hand sides, sweep, write the blocks.  trow_ptr / trow: per tile position t the
// positions s < t with a structurally non-zero factor tile L(t, s), ascending.  Enqueue only.
void launch_cov_batch(const DevProblem &d, int lcur, int cur, int ncb, const int *trow_ptr, const int *trow,
                      const CovGroup *groups, int ng, double *Zw, int bw, double *out_pose,
                      double *out_pt, hipStream_t s);

// ---- covariance blocks and the gate of a pose graph (ba_graph_kernels.hip) ----
struct PgCovGroup;  // ba_pgraph_host.h: one wave's two poses, pair or candidate
// Device outputs of one call, W x W doubles per block and W per residual: pose per distinct selected
// pose; rel (Sigma_E), cross (Sigma_jk, or null: not asked for) per pair or candidate; r / innov
// (or null) and d2 per candidate.
struct GraphCovOut {
  double *pose, *cross, *rel, *r, *innov, *d2;
};
// One column batch on the factored image of the graph (p.L, Ldiag; lambda = 0): zero the workspace
// Zw (p.npad x bw doubles, row-major, bw = 16 ng), place the identity columns, sweep, write the
// blocks.  poses: the accepted pose buffer; cand_val: the group's doubles per candidate as its
// pack_values lays them out (ba_rel_host.h, ba_sim3_host.h) or null; trow_ptr / trow as for
// launch_cov_batch.  Enqueue only.  (Called by graph_cov_run of ba_graph.hip through the kind's
// GraphSpec.)
template <class G>
void launch_graph_cov_batch(const PgDev &p, const double *Ldiag, int nb, int ncb, const double *poses,
                            const int *trow_ptr, const int *trow, const PgCovGroup *groups, int ng,
                            const double *cand_val, double *Zw, int bw, const GraphCovOut &out, hipStream_t s);

// ---- pose-only (ba_pose_only.hip) ----
struct PoIter {
  float cost, cost_change, abs_step;
};
int pose_only_sync_ints();       // size of the grid-barrier words (ints)
int pose_only_partial_floats();  // size of the partial-sum exchange buffer (floats)
int pose_only_mono6_device(const float *dX3, const float *duv2, int n, float fx,
                           float fy, float cx, float cy, float *dT12,
                           uint8_t *dmask, float thr_huber, float thr_step,
                           float thr_cost, float thr_out, int max_it,
                           PoIter *d_iters, int cap, int *d_meta,
                           float *d_debug, int *d_gsync, float *d_partial, hipStream_t s);
int pose_only_stereo6_device(const float *dX3, const float *duvl2, const float *duvr2, int n,
                             float fx, float fy, float cx, float cy, const float *d_cam_r16,
                             float *dT12, uint8_t *dmask_l, uint8_t *dmask_r, float thr_huber,
                             float thr_step, float thr_cost, float thr_out, int max_it,
                             PoIter *d_iters, int cap, int *d_meta, float *d_debug,
                             int *d_gsync, float *d_partial, hipStream_t s);
// B independent 6-DoF problems, one workgroup each (k_pose_only6<STEREO, true>);
// device pointers laid out as in ba_pose_only_{mono,stereo}6_batch_device
// (d_camr16 = B right-camera records, stereo only; d_res = B ba_po_result).
// Enqueue only.
int pose_only6_batch_device(bool stereo, int B, const int *d_offsets, const float *dX3,
                            const float *duvl2, const float *duvr2, const float *d_intr_l4,
                            const float *d_camr16, float *dT12, uint8_t *dmask_l, uint8_t *dmask_r,
                            float thr_huber, float thr_step, float thr_cost, float thr_out,
                            int max_it, PoIter *d_iters, int cap, int *d_res, float *d_debug,
                            hipStream_t s);
// planar 3-DoF (reference core/pose_only_bundle_adjustment_solver.cpp:401-900):
// everything the host derives in fp32 from the poses, passed by value
struct Po3Params {
  float theta0[3];       // prior (x, y, psi) of pose_b2b1
  float Rcb[9], tcb[3];  // camera_to_base = base_to_camera^-1 (left camera)
  float Rbc[9], tbc[3];  // base_to_camera (write-back)
  float Rrl[9], trl[3];  // right_to_left = left_to_right^-1 (stereo)
  float Rrb[9];          // R_rl * R_cb: the right camera's Jacobian rotation (:678-679)
  float cam_r[4];        // right fx, fy, cx, cy (stereo)
};
// the 52-float planar record of ba_planar_record / the batched planar solvers
static_assert(sizeof(Po3Params) == 52 * sizeof(float), "Po3Params must be 52 floats");
int pose_only_planar3_device(bool stereo, const float *dX3, const float *duvl2,
                             const float *duvr2, int n, float fx, float fy, float cx, float cy,
                             const Po3Params &P, float *dT12, uint8_t *dmask_l, uint8_t *dmask_r,
                             float thr_huber, float thr_step, float thr_cost, float thr_out,
                             int max_it, PoIter *d_iters, int cap, int *d_meta, float *d_debug,
                             int *d_gsync, float *d_partial, hipStream_t s);
// B independent planar problems, one workgroup each (k_pose_only3<STEREO, true>);
// device pointers laid out as in ba_pose_only_{mono,stereo}3_batch_device
// (d_rec52 = B Po3Params records; d_res = B ba_po_result).  Enqueue only.
int pose_only3_batch_device(bool stereo, int B, const int *d_offsets, const float *dX3,
                            const float *duvl2, const float *duvr2, const float *d_intr_l4,
                            const float *d_rec52, float *dT12, uint8_t *dmask_l, uint8_t *dmask_r,
                            float thr_huber, float thr_step, float thr_cost, float thr_out,
                            int max_it, PoIter *d_iters, int cap, int *d_res, float *d_debug,
                            hipStream_t s);

}  // namespace ba
#endif
