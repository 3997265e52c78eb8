/*
 * ba_hip.h — C ABI of the MI355X (gfx950) bundle-adjustment hot path.
 *
 * The reference has no FFI / plugin layer: its boundary is the C++ class
 * FullBundleAdjustmentSolver (reference core/full_bundle_adjustment_solver.h:
 * 127-146) whose Solve() (reference core/full_bundle_adjustment_solver.cpp:
 * 630-1044) is the hot path.  This header is the thin C ABI a replacement
 * facade binds: plain pointers and sizes, an opaque handle,
 * no C++ or torch types.  Every entry point names the reference lines it
 * replaces.  Conventions:
 *   - return 0 = OK, negative = error (message via ba_last_error()); no C++
 *     exception crosses the ABI;
 *   - caller-owned HOST arrays are copied at set_* time;
 *   - all values are in the solver's SCALED units: the facade applies the
 *     reference's 0.01 scaling (reference :38, :74-79, :97, :113, :176),
 *     inverts user poses into T_jw (reference :96) and maps pointers to
 *     indices before calling in;
 *   - rigid transforms are 12 doubles: row-major 3x3 rotation, then t;
 *   - one handle per host thread; a handle owns one GPU.
 */
#ifndef BA_HIP_H_
#define BA_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ba_handle ba_handle;

/* Mirrors Options (reference core/solver_option_and_summary.h:47-71); the
 * fields are float there and are promoted to double inside the LM update
 * (reference core/full_bundle_adjustment_solver.cpp:949,953). */
typedef struct {
  float threshold_step_size;         /* convergence_handle  */
  float threshold_cost_change;       /* convergence_handle  */
  float threshold_huber_loss;        /* outlier_handle      */
  float threshold_outlier_rejection; /* unused by full BA   */
  int max_num_iterations;            /* iteration_handle    */
  float initial_lambda;              /* trust_region_handle */
  float decrease_ratio_lambda;
  float increase_ratio_lambda;
  /* 1 = plain Gauss-Newton of FullBundleAdjustmentSolverRefactor (reference
   * core/full_bundle_adjustment_solver_refactor.cpp:976-982: every step
   * accepted, lambda fixed at initial_lambda); 0 = Levenberg-Marquardt, the
   * only mode of FullBundleAdjustmentSolver::Solve (its solver_type is
   * ignored, reference :630-1044). */
  int gauss_newton;
} ba_options;

/* One row per LM iteration: OptimizationInfo (reference
 * core/solver_option_and_summary.h:37-46) + the trust-region internals. */
typedef struct {
  double cost;
  double cost_change;
  double average_reprojection_error;
  double abs_gradient;
  double abs_step;
  double damping_term;
  double iter_time_ms;
  int iteration_status; /* 0 UPDATE, 1 UPDATE_TRUST_MORE, 2 SKIPPED */
  int pad_;
  double rho;
  double model_change;
  double trial_cost;
} ba_iter_info;

/* ---- lifetime --------------------------------------------------------- */
/* replaces the constructor / destructor / Reset (reference :6-70) */
int ba_create(ba_handle **out, int device_id);
void ba_destroy(ba_handle *h);
const char *ba_last_error(void);
/* Run all kernels of this handle on the given hipStream_t (used as is: NULL
 * is HIP's default stream).  Without this call the handle uses a stream of
 * its own. */
int ba_set_stream(ba_handle *h, void *hip_stream);

/* ---- problem construction (host arrays, copied) ------------------------ */
/* AddCamera, reference :72-85.  intr4 = fx,fy,cx,cy ; T_cj12 = body->camera */
int ba_set_cameras(ba_handle *h, int n_cam, const double *intr4,
                   const double *T_cj12);
/* AddPose + MakePoseFixed, reference :87-101, :119-134.  T_jw = pose^-1 */
int ba_set_poses(ba_handle *h, int n_pose, const double *T_jw12,
                 const uint8_t *fixed);
/* AddPoint + MakePointFixed, reference :103-117, :136-153 */
int ba_set_points(ba_handle *h, int n_pt, const double *X3,
                  const uint8_t *fixed);
/* AddObservation, reference :155-180.  Insertion order is preserved: it
 * decides which camera's cross term B_ji survives (reference :826). */
int ba_set_observations(ba_handle *h, int64_t n_obs, const int32_t *cam,
                        const int32_t *pose, const int32_t *point,
                        const double *uv2);
/* Landmark-range sharding for multi-GPU (new).  Call before
 * ba_finalize with the same full problem on every rank. */
int ba_set_shard(ba_handle *h, int rank, int world);
/* FinalizeParameters + SetProblemSize + connectivity, reference :182-206,
 * :243-308, :668-700: index assignment, block-sparse structure, upload. */
int ba_finalize(ba_handle *h);

/* New VALUES for the same STRUCTURE (a SLAM back end re-optimising the same graph):
 * replaces the parameters of a finalized problem — T_jw12 for all n_pose poses
 * and / or X3 for all n_pt points in user order, NULL = keep — without planning
 * again (index assignment, block structure, schedules and uploads of ba_finalize
 * stay: 0.2-0.6 s at BASELINE config C4).  Fixed flags, cameras and observations
 * cannot change.  The next ba_solve / ba_lm_begin starts from the new values.  (The
 * reference keeps its registered state across Solve calls, :44-70, and has no way
 * to re-seed it short of Reset.) */
int ba_update_values(ba_handle *h, const double *T_jw12, const double *X3);

/* Relative-pose factors on the handle path: odometry and loop-closure edges between the
 * poses of a resident problem of any size.  The definition is
 * ba_batch_set_relative's, word for word: factor f names two distinct poses rel_j[f],
 * rel_k[f] by user index, at least one of them optimisable, a measurement Z (12 doubles,
 * scaled units) of T_j T_k^-1 and a 6x6 information matrix Omega (36 doubles, row-major; only
 * the lower triangle is read and mirrored).  r = se3_log(T_j T_k^-1 Z^-1), Jacobians I and
 * -Ad(T_j T_k^-1):
 *   A_j += Omega,  A_k += Ad^T Omega Ad,  S_jk += -Omega Ad,  a_j += -Omega r,  a_k += Ad^T Omega r.
 * A fixed pose receives nothing.  The diagonal contributions join A_j before the damping, the
 * off-diagonal block joins S undamped, the model gains 2 x_j^T S_jk x_k, every cost (initial,
 * trial, ba_stage_cost) gains sqrt(max(0, r^T Omega r)) per factor; n_obs and the block count
 * of the average step do not change; no robust weight.  Several factors may name one pair, in
 * either orientation: they are summed in input order.  No cap on factors.  Every pair of two
 * optimisable poses becomes a block of S (and couples their tiles in the factor's pattern)
 * whether or not the two poses share a landmark; a pose without observations is held by its
 * factors alone.  ba_solve / ba_lm_*, every ba_stage_* call and ba_covariance include the
 * factors; ba_get_A / ba_get_S show the blocks with them.
 * Call before ba_finalize (the factors change the structure); afterwards the call is refused.
 * n_rel == 0, or every array NULL, clears.  Validation happens before anything touches the GPU,
 * with the rules and messages of ba_batch_set_relative (-1 and ba_last_error, naming the
 * factor): indices in range (ba_set_poses comes first), j != k, not both fixed, every value
 * finite.  A refused call changes nothing.  ba_finalize checks the pairs once more against
 * the poses it finds.
 * Refused on a handle that holds factors, in whichever order the calls arrive: sharding
 * (ba_set_shard with world > 1, ba_set_allreduce), gradient descent (ba_gd_*, ba_solve_gd) and
 * BA_GRAPH=1 replay.  ba_stream_* takes no factors.  A handle without factors launches exactly
 * the kernels it launched before.  One writer per element, fixed summation order, no
 * floating-point atomics: the same bits run to run. */
int ba_set_relative(ba_handle *h, int64_t n_rel, const int32_t *rel_j, const int32_t *rel_k,
                    const double *Z12, const double *Omega36);
/* New VALUES (Z, Omega) for the same pairs on a finalized handle, without planning again: the
 * companion of ba_update_values, which keeps the factors.  Both arrays hold one entry per
 * factor given to ba_set_relative; validated as there.  The next ba_solve / ba_lm_begin
 * linearises with the new values. */
int ba_update_relative(ba_handle *h, const double *Z12, const double *Omega36);
/* Host-only (no GPU): the validation of ba_set_relative for n_pose poses with the flags
 * pose_fixed (NULL: none fixed).  0, or -1 and ba_last_error. */
int ba_relative_check(int n_pose, const uint8_t *pose_fixed, int64_t n_rel, const int32_t *rel_j,
                      const int32_t *rel_k, const double *Z12, const double *Omega36);
/* out4 = { factors, blocks of S that carry a factor, blocks of S that exist only because of a
 * factor, device bytes of the factor records plus both scratch buffers }; before ba_finalize
 * the last three are 0. */
int ba_relative_info(ba_handle *h, int64_t out4[4]);

/* Host-only helper (no GPU needed): owner rank of every point under the
 * sharding rule used by ba_finalize. */
int ba_partition_points(int n_pose, const uint8_t *pose_fixed, int n_pt,
                        const uint8_t *pt_fixed, int64_t n_obs,
                        const int32_t *obs_pose, const int32_t *obs_pt,
                        int world, int32_t *owner_out);

/* ---- multi-GPU exchange hook ------------------------------------------- */
/* The caller owns the collective (RCCL through torch.distributed, or
 * anything else).  `which`: 0 = reduced camera system, PACKED: the 36 entries
 * of every structurally non-zero 6x6 block of S (global block numbering,
 * identical on all shards) followed by the 6N entries of rhs; 1 = LM scalars.
 * The hook must sum-all-reduce n doubles at dev_ptr in place, ordered on
 * hip_stream. */
typedef int (*ba_allreduce_fn)(void *user, int which, void *dev_ptr,
                               int64_t n_doubles, void *hip_stream);
int ba_set_allreduce(ba_handle *h, ba_allreduce_fn fn, void *user);
/* `which` = 2 (ba_gather_points only): every point of the FULL problem in user
 * order, 3 doubles each, the rows of points this shard does not own zero. */
/* Size (in doubles) of exchange buffer `which` (0, 1 or 2), valid after ba_finalize. */
int64_t ba_reduce_buffer_size(ba_handle *h, int which);
/* Use caller-allocated DEVICE memory for exchange buffer `which` (so that a
 * framework tensor can alias it).  Call after ba_finalize. */
int ba_bind_reduce_buffer(ba_handle *h, int which, void *dev_ptr,
                          int64_t n_doubles);

/* Write-back under sharding.  The reference updates EVERY registered, non-fixed
 * point through the caller's pointer at the end of Solve (reference :1018-1022);
 * a shard holds the final values of the landmarks it owns only.  This call
 * sum-all-reduces the owned rows (hook, which = 2: 12 MB at BASELINE config C4,
 * once per Solve); afterwards, and until the next ba_lm_begin / ba_lm_iterate /
 * ba_stage_commit, ba_get_points returns every point of the full problem
 * (owned_mask all 1) on every rank.  A no-op without a hook or with world = 1. */
int ba_gather_points(ba_handle *h);

/* ---- RCCL exchange (csrc/ba_rccl.cpp) ----------------------------------- */
/* The hook above implemented over RCCL inside the library, so that no host
 * language runs between the kernels of an LM iteration: rank 0 draws the 128-byte
 * communicator id and hands it to the other ranks by any side channel (a file,
 * MPI, a torch.distributed broadcast); every rank creates its communicator and
 * registers  ba_set_allreduce(h, ba_rccl_allreduce_hook, comm).  librccl is
 * bound with dlopen at the first call (BA_RCCL_LIB, else librccl.so.1 — the copy
 * already in the process if a framework brought one). */
typedef struct ba_rccl_comm ba_rccl_comm;
int ba_rccl_available(void);                         /* 1 / 0 (reason: ba_last_error) */
int ba_rccl_get_unique_id(uint8_t id128[128]);       /* ncclGetUniqueId */
int ba_rccl_comm_create(ba_rccl_comm **out, int rank, int world,
                        const uint8_t id128[128], int device_id);
int ba_rccl_comm_size(ba_rccl_comm *c);              /* ranks the communicator sees (ncclCommCount) */
int64_t ba_rccl_comm_calls(ba_rccl_comm *c);         /* all-reduces issued so far */
void ba_rccl_comm_destroy(ba_rccl_comm *c);
/* a ba_allreduce_fn; user = ba_rccl_comm* */
int ba_rccl_allreduce_hook(void *user, int which, void *dev_ptr,
                           int64_t n_doubles, void *hip_stream);

/* ---- the LM loop ------------------------------------------------------- */
/* Solve, reference :630-1044 (iteration loop :705-1008).  Runs until
 * convergence or max_num_iterations; fills up to `cap` rows. */
int ba_solve(ba_handle *h, const ba_options *opt, ba_iter_info *out, int cap,
             int *n_iter, int *converged);
/* The same loop in three asynchronous pieces (bench / graph replay):
 * begin = lambda0 + initial cost (reference :707-708); iterate = enqueue n
 * LM iterations without host synchronisation (iterations after convergence
 * are device-side no-ops); sync = wait and read the iteration log. */
int ba_lm_begin(ba_handle *h, const ba_options *opt);
int ba_lm_iterate(ba_handle *h, int n);
/* returns 1 when the loop has finished, 0 when not, < 0 on error — also when a
 * dataflow hand-off of the reduced solve timed out on the device (the sweeps of
 * csrc/ba_dense_tile.inc poll with a bound; x is then partly unsolved and every
 * iteration since ba_lm_begin is invalid; ba_last_error names it). */
int ba_lm_sync(ba_handle *h, ba_iter_info *out, int cap, int *n_iter,
               int *converged);

/* ---- gradient descent ----------------------------------------------------- */
/* FullBundleAdjustmentSolverRefactor::SolveByGradientDescent, reference
 * core/full_bundle_adjustment_solver_refactor.cpp:1075-1367: per iteration
 * a_j = -sum Q_ij^T w r_ij (optimisable poses), b_i = -sum R_ij^T w r_ij
 * (optimisable points), each block clipped to norm <= 1e-3 (scaled units),
 * T_jw <- exp(a_j) T_jw and X_i <- X_i + b_i, every step taken.  The rows:
 * cost = sum ||r|| at the new parameters (every observation), cost_change =
 * |cost - previous|, average_reprojection_error = cost / observations (no
 * sqrt), abs_step = (0.01 + sum ||a_j|| + 0.01 + sum ||b_i||) / (N + M) of
 * the clipped blocks, abs_gradient = 0, damping_term = initial_lambda,
 * iteration_status = UPDATE, rho = 0, model_change = 0, trial_cost = cost.
 * Stop: converged if abs_step < threshold_step_size or cost_change <
 * threshold_cost_change, never on the last allowed iteration.  gauss_newton,
 * decrease_ratio_lambda and increase_ratio_lambda are ignored.  Single GPU:
 * a sharded handle (ba_set_shard world > 1, or an all-reduce hook) is refused.
 * The parameters are updated in place: ba_get_poses / ba_get_points return
 * the GD result and a following ba_solve starts from it.  The same
 * begin / iterate / sync split as the LM loop; ba_lm_iterate after
 * ba_gd_begin and ba_gd_iterate after ba_lm_begin fail. */
int ba_gd_begin(ba_handle *h, const ba_options *opt);   /* :1109-1158 */
int ba_gd_iterate(ba_handle *h, int n);                 /* enqueue n iterations */
/* returns 1 when the loop has finished, 0 when not, < 0 on error */
int ba_gd_sync(ba_handle *h, ba_iter_info *out, int cap, int *n_iter,
               int *converged);
int ba_solve_gd(ba_handle *h, const ba_options *opt, ba_iter_info *out,
                int cap, int *n_iter, int *converged);  /* :1075-1367 */
/* the unclipped gradient at the current parameters (computed by the last pass
 * over the observations: after ba_gd_begin the starting point's), in the order
 * and layout of ba_get_A's a6 and ba_get_C's b3 */
int ba_gd_get_gradient(ba_handle *h, double *a6, double *b3);

/* ---- stage entry points (parity tests, per-stage timing) --------------- */
int ba_stage_cost(ba_handle *h, double *cost);            /* :381-433 */
int ba_stage_linearize(ba_handle *h, double lambda,
                       double huber);                     /* :716-856 */
int ba_stage_schur(ba_handle *h);                         /* :858-902 */
int ba_stage_solve_reduced(ba_handle *h);                 /* :905-908 */
int ba_stage_backsub_update(ba_handle *h);  /* :910-926, :435-455, :960-963 */
/* after ba_stage_backsub_update: trial cost, model change, step norms */
int ba_stage_scalars(ba_handle *h, double *trial_cost, double *model_change,
                     double *pose_step_sum, double *point_step_sum);
/* accept (1) or reject (0) the trial parameters, reference :939-945 */
int ba_stage_commit(ba_handle *h, int accept);

/* Accumulated device time per stage in ms since the last reset (hipEvents;
 * enabled by ba_enable_stage_timing): [0] build (linearize), [1] schur,
 * [2] reduced solve, [3] backsub+update, [4] cost, [5] control,
 * [6] exchange (all-reduce hook), [7] reserved. */
int ba_enable_stage_timing(ba_handle *h, int on);
int ba_get_stage_ms(ba_handle *h, double out8[8], int reset);

/* ---- readers (user index order; opt order = input order of non-fixed) -- */
int ba_num_opt_poses(ba_handle *h);
int ba_num_opt_points(ba_handle *h); /* local (owned) optimisable points */
int64_t ba_num_pairs(ba_handle *h);
int64_t ba_num_schur_blocks(ba_handle *h);
int64_t ba_num_schur_triples(ba_handle *h);
/* current parameters, write-back source (reference :1011-1022) */
int ba_get_poses(ba_handle *h, double *T_jw12 /* n_pose*12 */);
/* points not owned by this shard are left untouched; owned_mask may be NULL */
int ba_get_points(ba_handle *h, double *X3 /* n_pt*3 */, uint8_t *owned_mask);
/* damped A_j (6x6 full) and a_j, per optimised pose */
int ba_get_A(ba_handle *h, double *A36, double *a6);
/* damped C_i (3x3 full), b_i; Cinv_i, Cinv_i b_i.  Indexed by GLOBAL opt
 * point index; entries of points owned by other shards are left untouched */
int ba_get_C(ba_handle *h, double *C9, double *b3);
int ba_get_Cinv(ba_handle *h, double *Cinv9, double *Cinvb3);
/* pairs (global i_opt, j_opt) in internal order with W = B_ji (6x3, row-major; the
 * device keeps it compact as {K, X_ij} and this call expands it) */
int ba_get_pairs(ba_handle *h, int32_t *pair_i, int32_t *pair_j, double *W18);
/* Host-side step of ba_get_pairs, no device involved: the pairs of covisibility groups
 * are kept as rec8 = {G (2x3 row-major), w, 0} of the pair's last writer; with the pose
 * T12 = {R_jw row-major, t_jw} and the point X3 the blocks were linearised at this gives
 * k12 = {K = G^T w G R_jw (3x3 row-major), X_ij = R_jw X + t_jw}, the compact form of
 * every other pair.  The group kernels rebuild K and X_ij by the same expression. */
void ba_expand_pair_slim(const double *rec8, const double *T12, const double *X3, double *k12);
/* reduced camera system, (6N)^2 row-major, and rhs, in opt-pose order */
int ba_get_S(ba_handle *h, double *S, double *rhs);
int ba_get_xy(ba_handle *h, double *x6, double *y3);

/* Per-kernel device time (hipEvents around every launch, recorded on the
 * handle's stream) accumulated while stage timing is enabled: total ms and
 * number of launches per kernel id in [0, ba_kernel_count()). */
int ba_kernel_count(void);
const char *ba_kernel_name(int id);
int ba_get_kernel_ms(ba_handle *h, double *ms_out, int64_t *calls_out, int reset);

/* Structure of the reduced-system factorisation chosen at ba_finalize:
 * out4 = { non-zero tile fraction of the factor (1 = dense), executed flop
 * estimate per solve, number of elimination levels (launch depth), padded
 * matrix order }. */
int ba_get_dense_info(ba_handle *h, double out4[4]);

/* How the Schur complement of this shard is accumulated (chosen at ba_finalize):
 * out8 = { workgroups of the covisibility-group kernel with 32-wide tiles (pose
 * sets of <= 5 poses), the same with 64-wide tiles (6..10 poses), landmarks
 * covered by groups, super-runs (the other landmarks), (landmark, pose) pairs in
 * groups, Schur triples in groups, v_mfma_f64_16x16x4 instructions the group
 * kernel executes per launch, triples on the global list (landmarks too large
 * for a super-run) }. */
int ba_get_schur_info(ba_handle *h, int64_t out8[8]);

/* How this shard is linearised and back-substituted (chosen at ba_finalize):
 * out4 = { workgroups (pieces) of the covisibility-group linearisation kernel —
 * landmark and pose side of the grouped landmarks in one pass; 0 if the groups
 * are linearised by the chunk / pose-major kernels —, observations those pieces
 * cover, landmark chunks left to the chunk kernel, observations on the
 * pose-major list }. */
int ba_get_lin_info(ba_handle *h, int64_t out4[4]);
/* Pair records of this shard: out2 = { pairs kept as the 64-byte record {G, w} (the pairs of
 * the covisibility groups, when k_lin_grp linearises them and BA_PAIR_SLIM is not 0), all
 * pairs, padded ones included }.  The others keep the 96-byte record {K, X_ij}. */
int ba_get_pair_record_info(ba_handle *h, int64_t out2[2]);
/* The record form of the grouped pairs that this handle took at ba_finalize: 0 = the 96-byte
 * record, 1 = the slim record {G, w}, 2 = "from the observation": the iteration keeps no
 * record of them, the group kernels rebuild {G, w} from the observation of the pair's last
 * writer (slim handles whose groups are all 32 wide and unmasked; BA_PAIR_OBS=0 keeps 1). */
int ba_get_pair_form(ba_handle *h);
/* The slim records rec8 (8 doubles each) of the first out2[0] pairs of
 * ba_get_pair_record_info as the device holds them (form 2: as k_pair_records fills them on
 * demand), with each pair's pose and point (the caller's indices) and, for the pairs of unmasked
 * groups, the camera and uv of its last writer.  Any output may be NULL. */
int ba_get_slim_records(ba_handle *h, int32_t *pose, int32_t *lm, int32_t *cam, double *uv2, double *rec8);
/* Host side of form 2, no device involved: rec8 = {G, w, 0} of one observation from its
 * camera (16 doubles), the pose T12, the point X3, uv2 and the Huber threshold, with the
 * bits k_lin_grp computes for that observation. */
void ba_pair_G_from_obs(const double *cam16, const double *T12, const double *X3, const double *uv2, double huber,
                        double *rec8);

/* Superset ("masked") covisibility groups — landmarks of one pose span whose
 * observation patterns differ (occlusion, image borders, track loss) share the UNION
 * of their patterns; a member's missing observations are padded slots of weight 0, its
 * missing pairs zero W records: out4 = { k_lin_grp pieces of masked groups, landmarks
 * in masked groups, padded observation slots, padded (landmark, pose) pairs }.  The
 * padding is internal: ba_num_pairs / ba_get_pairs do not show it. */
int ba_get_mask_info(ba_handle *h, int64_t out4[4]);

/* The reduced system is factorised by Cholesky WITHOUT pivoting; the
 * reference uses Eigen's diagonally pivoted LDLT with a pseudo-inverted D
 * (reference :905).  A non-positive pivot (<= 1e-300: a pose without
 * observations, or an indefinite / rank-deficient S, e.g. no fixed pose and
 * lambda at its floor) zeroes its column and solution component instead.
 * `count` receives how many such pivots the factorisations met since
 * ba_lm_begin (or since the last reset): 0 means the two factorisations agree
 * up to roundoff.  (Timed-out hand-offs of the dataflow sweeps are NOT counted
 * here: they are errors, reported by ba_lm_sync.) */
int ba_get_dropped_pivots(ba_handle *h, int64_t *count, int reset);

/* ---- observation streaming: problems larger than device memory ---------- */
/* SURVEY.md 8f N4 (the reference has no counterpart: its dense N x M grids stop it
 * at 62 GB of host memory long before).  The landmarks are cut into n_chunks
 * chunks by the rule of ba_set_shard; a chunk's observations, W = B_ji, C_i, b_i and
 * points live in ONE of two device arenas of arena_bytes each and in a pinned host
 * image otherwise; per LM iteration every chunk passes through the device twice
 * (Schur accumulation; back-substitution + trial-point linearisation), its
 * transfers overlapped with the kernels of the chunk before it.  Poses, the packed
 * partial S||rhs and the controller are resident per chunk, the dense image and x
 * once.  Same problem-construction calls, same options and iteration rows as
 * ba_solve; the trajectory equals the resident solve up to the summation order of
 * the chunks' partial sums.  ba_stream_finalize fails if a chunk does not fit the
 * arena ("use more chunks"). */
typedef struct ba_stream ba_stream;
int ba_stream_create(ba_stream **out, int device_id, int n_chunks, int64_t arena_bytes);
void ba_stream_destroy(ba_stream *s);
int ba_stream_set_cameras(ba_stream *s, int n_cam, const double *intr4, const double *T_cj12);
int ba_stream_set_poses(ba_stream *s, int n_pose, const double *T_jw12, const uint8_t *fixed);
int ba_stream_set_points(ba_stream *s, int n_pt, const double *X3, const uint8_t *fixed);
int ba_stream_set_observations(ba_stream *s, int64_t n_obs, const int32_t *cam, const int32_t *pose,
                               const int32_t *point, const double *uv2);
int ba_stream_finalize(ba_stream *s);
int ba_stream_solve(ba_stream *s, const ba_options *opt, ba_iter_info *out, int cap,
                    int *n_iter, int *converged);
/* the same loop in three pieces, like ba_lm_begin / ba_lm_iterate / ba_lm_sync */
int ba_stream_lm_begin(ba_stream *s, const ba_options *opt);
int ba_stream_lm_iterate(ba_stream *s, int n);
int ba_stream_lm_sync(ba_stream *s, ba_iter_info *out, int cap, int *n_iter, int *converged);
int ba_stream_get_poses(ba_stream *s, double *T_jw12);
int ba_stream_get_points(ba_stream *s, double *X3);
/* out6 = { device bytes of the arenas, bytes of the largest chunk, bytes of all
 * chunks together (what a resident solve would hold), bytes copied host->device and
 * device->host since ba_stream_finalize, number of chunks } */
int ba_stream_info(ba_stream *s, int64_t out6[6]);

/* ---- dense SPD solve alone (tests / micro-bench of the MFMA kernel) ---- */
/* Solves A x = b for symmetric positive (semi-)definite A (n x n row-major
 * host arrays) with the blocked fp64-MFMA Cholesky used for the reduced
 * camera system.  `ms` (optional) receives the device time of the solve. */
int ba_dense_spd_solve(ba_handle *h, int n, const double *A, const double *b,
                       double *x, double *ms);

/* ---- covariance blocks from the factored reduced camera system ---------- */
/* How well the current accepted values are determined (the reference has no
 * counterpart; Ceres' Covariance, g2o's computeMarginals, GTSAM's Marginals).
 * The call linearises at the current accepted values with lambda = 0 and the
 * given Huber threshold, forms, scatters and factorises the Schur complement S
 * with the launches of ba_stage_linearize(0, huber), ba_stage_schur and the
 * factor half of ba_stage_solve_reduced, and reads the blocks off the factor
 * S = L L^T (csrc/ba_cov.hip, fp64 MFMA, no atomics: the same bits every run):
 *   cov_pose36[s]  the 6x6 row-major block [S^-1]_jj of pose pose_sel[s];
 *   cov_pt9[s]     Sigma_ii = Cinv_i + Cinv_i W_i^T Sigma_P(i) W_i Cinv_i of point
 *                  pt_sel[s], Sigma_P(i) = ALL blocks of S^-1, off-diagonal ones
 *                  included, among the poses paired with landmark i.
 * Both are blocks of the inverse of the solver's own normal matrix
 * [[A, W], [W^T, C]], in the solver's scaled units; pose tangent xi = [v; omega]
 * of T_jw <- exp(xi) T_jw (world-to-body, left-multiplicative).  pose_sel /
 * pt_sel are USER indices of optimisable poses / points, in any order, repeats
 * allowed; either selection may be empty and its output pointer then NULL.
 * dropped_pivots (may be NULL) receives the non-positive pivots THIS call's
 * factorisation met; the count of ba_get_dropped_pivots is not disturbed.
 *  - Poses, points, the accepted-buffer index and the LM / GD controller are
 *    untouched: ba_solve after ba_covariance gives the bits it gives without.
 *    The stage intermediates (ba_get_A, ba_get_C, ba_get_pairs, ba_get_S, ...)
 *    hold the lambda = 0 linearisation afterwards (ba_get_A / ba_get_C apply
 *    the controller's lambda, which the call restores).
 *  - Stereo: the matrix inverted is the solver's normal matrix, with the
 *    last-writer rule of the cross block W_ji (one camera's J^T W J plus
 *    block-diagonal terms: positive semi-definite, but not the full two-camera
 *    J^T W J).  In mono the two coincide.
 *  - A never-observed landmark has Cinv = 0 and no pairs: its block is exactly
 *    zero.  A rank-deficient C_i gets what the solver's pseudo-inverse yields.
 *  - Without a fixed pose S is singular at lambda = 0 and the result
 *    meaningless: dropped_pivots > 0 is how the caller learns of it.
 * Returns -1 (ba_last_error), before anything touches the device, if the handle
 * is not finalized, is sharded (ba_set_shard world > 1 or an all-reduce hook) or
 * streamed, an index is out of range or names a fixed pose / point, or an output
 * pointer is NULL for a non-empty selection.
 * The right-hand sides (6 per distinct pose, 3 per distinct point, 16 per wave)
 * are processed in column batches; the workspace, npad x batch x 8 bytes, is
 * allocated on the handle and freed on return. */
int ba_covariance(ba_handle *h, double huber,
                  int n_pose_sel, const int32_t *pose_sel, double *cov_pose36,
                  int n_pt_sel, const int32_t *pt_sel, double *cov_pt9,
                  int64_t *dropped_pivots);
/* out4 = { columns of one batch on this handle (what fits 256 MiB of workspace,
 * at most 16384; BA_COV_BATCH=<columns> overrides), columns per wave (16: two
 * poses or five points), bytes of the workspace at that width, batches the last
 * ba_covariance ran } */
int ba_covariance_info(ba_handle *h, int64_t out4[4]);
/* The argument checks of ba_covariance on plain values (host only, no device):
 * finalized / sharded / streamed flags, the fixed masks of the n_pose poses and
 * n_pt points (NULL: none fixed), the selections and output pointers.  0 or -1. */
int ba_covariance_check(int finalized, int sharded, int streamed, int n_pose,
                        const uint8_t *pose_fixed, int n_pt, const uint8_t *pt_fixed,
                        int n_pose_sel, const int32_t *pose_sel, const double *cov_pose36,
                        int n_pt_sel, const int32_t *pt_sel, const double *cov_pt9);

/* ---- pose-only, monocular 6-DoF (fp32) --------------------------------- */
/* Solve_Monocular_6Dof, reference
 * core/pose_only_bundle_adjustment_solver.cpp:8-170.  T12 in/out is
 * reference_to_current_pose; mask is n bytes in/out (sticky false). */
typedef struct {
  float cost, cost_change, abs_step;
} ba_po_iter;
int ba_pose_only_mono6(ba_handle *h, const float *X3, const float *uv2, int n,
                       float fx, float fy, float cx, float cy, float *T12,
                       uint8_t *mask, const ba_options *opt, ba_po_iter *iters,
                       int cap, int *n_iter, int *converged,
                       float *debug_T12);

/* ---- pose-only, stereo 6-DoF (fp32) ------------------------------------- */
/* Solve_Stereo_6Dof, reference
 * core/pose_only_bundle_adjustment_solver.cpp:172-399.  intr_*4 = fx,fy,cx,cy;
 * T_lr12 = left_to_right_pose; T12 in/out = reference_to_current_left_pose;
 * a right pixel with a negative coordinate means "no right observation"
 * (:298); mask_l / mask_r are n bytes each, in/out (sticky false). */
int ba_pose_only_stereo6(ba_handle *h, const float *X3, const float *uvl2,
                         const float *uvr2, int n, const float *intr_l4,
                         const float *intr_r4, const float *T_lr12, float *T12,
                         uint8_t *mask_l, uint8_t *mask_r, const ba_options *opt,
                         ba_po_iter *iters, int cap, int *n_iter, int *converged,
                         float *debug_T12);

/* ---- pose-only, planar 3-DoF (fp32), monocular and stereo ----------------- */
/* Solve_Monocular_Planar3Dof / Solve_Stereo_Planar3Dof, reference
 * core/pose_only_bundle_adjustment_solver.cpp:401-615 / :617-900.  The unknown
 * is (x, y, psi) of pose_b2b1 (base-1 -> base-2); its prior is
 * T_bc * (T12^-1 * T_wl) * T_bc^-1.  X3 are base-1 coordinates.  T_bc12 =
 * pose_base_to_camera, T_wl12 = pose_world_to_last, T12 in/out =
 * pose_world_to_current, written as pose_b2b1^-1 * T_bc after at least one
 * iteration when the pose is not NaN (else left unchanged, return 1).
 * max_num_iterations = 0: T12 unchanged, converged, no rows, return 0.
 * Stereo: intr_*4 = fx,fy,cx,cy; T_lr12 = left_to_right_pose; a right pixel
 * with a negative coordinate means "no right observation" (:785).  Masks are n
 * bytes each, in/out (sticky false). */
int ba_pose_only_mono3(ba_handle *h, const float *X3, const float *uv2, int n,
                       float fx, float fy, float cx, float cy,
                       const float *T_bc12, const float *T_wl12, float *T12,
                       uint8_t *mask, const ba_options *opt, ba_po_iter *iters,
                       int cap, int *n_iter, int *converged,
                       float *debug_T12);
int ba_pose_only_stereo3(ba_handle *h, const float *X3, const float *uvl2,
                         const float *uvr2, int n, const float *intr_l4,
                         const float *intr_r4, const float *T_bc12,
                         const float *T_lr12, const float *T_wl12, float *T12,
                         uint8_t *mask_l, uint8_t *mask_r, const ba_options *opt,
                         ba_po_iter *iters, int cap, int *n_iter, int *converged,
                         float *debug_T12);

/* ---- batched pose-only 6-DoF (fp32): many problems in one launch ---------- */
/* B independent Solve_Monocular_6Dof / Solve_Stereo_6Dof problems, one
 * 1024-thread workgroup each, no grid barrier (any B is safe).  Problem b owns
 * points [offsets[b], offsets[b+1]) of the concatenated X3 / uv2 (uvr2) / mask
 * arrays, intrinsics intr4 + 4b (intr_l4, intr_r4 for stereo), T_lr12 + 12b
 * (stereo), pose T12 + 12b (in/out), Summary rows iters + b*cap and debug poses
 * debug_T12 + 12*b*cap (both optional, at most cap rows each); one ba_options
 * for the whole batch.  res[b] receives its result.  A problem of n <= 2048
 * points gives bit for bit what the single call gives it; larger ones agree to
 * fp32 rounding (the single call spreads them over several workgroups, which
 * sums in another order, and is faster for them).  max_num_iterations <= 0:
 * every pose unchanged, converged, no rows.
 * Host arrays: B >= 1, offsets[0] == 0 and strictly increasing offsets are
 * checked first (else -1, nothing runs); one H2D copy, one launch, one D2H copy
 * and a sync on the handle's stream.  Returns 0 when every problem was
 * processed, whatever its status, and -1 on a runtime error. */
typedef struct {
  int n_iter, converged, n_rows, status;
  /* n_rows = Summary rows logged (rows stored: min(n_rows, cap));
   * status: 0 = pose written, 1 = NaN pose (input left unchanged, as the single
   * call's return 1), 2 = malformed problem (device entry points only:
   * offsets[b+1] <= offsets[b]; nothing else written) */
} ba_po_result;
int ba_pose_only_mono6_batch(ba_handle *h, int B, const int32_t *offsets,
                             const float *X3, const float *uv2,
                             const float *intr4, float *T12, uint8_t *mask,
                             const ba_options *opt, ba_po_iter *iters, int cap,
                             ba_po_result *res, float *debug_T12);
int ba_pose_only_stereo6_batch(ba_handle *h, int B, const int32_t *offsets,
                               const float *X3, const float *uvl2,
                               const float *uvr2, const float *intr_l4,
                               const float *intr_r4, const float *T_lr12,
                               float *T12, uint8_t *mask_l, uint8_t *mask_r,
                               const ba_options *opt, ba_po_iter *iters,
                               int cap, ba_po_result *res, float *debug_T12);
/* The same on DEVICE pointers (offsets and res included), enqueued on
 * hip_stream (NULL = the handle's stream) with no copy and no synchronisation;
 * only the pointers and B are checked on the host.  Stereo takes B prepared
 * right-camera records camr16 (B x 16, from ba_right_camera_record) instead of
 * intr_r4 and T_lr12. */
int ba_pose_only_mono6_batch_device(ba_handle *h, int B, const int32_t *offsets,
                                    const float *X3, const float *uv2,
                                    const float *intr4, float *T12,
                                    uint8_t *mask, const ba_options *opt,
                                    ba_po_iter *iters, int cap,
                                    ba_po_result *res, float *debug_T12,
                                    void *hip_stream);
int ba_pose_only_stereo6_batch_device(ba_handle *h, int B,
                                      const int32_t *offsets, const float *X3,
                                      const float *uvl2, const float *uvr2,
                                      const float *intr_l4, const float *camr16,
                                      float *T12, uint8_t *mask_l,
                                      uint8_t *mask_r, const ba_options *opt,
                                      ba_po_iter *iters, int cap,
                                      ba_po_result *res, float *debug_T12,
                                      void *hip_stream);
/* Host helper: the right-camera record of one stereo problem, {fx, fy, cx, cy
 * of intr_r4, then left_to_right^-1 as R (9, row-major) and t (3)}, with the
 * fp32 expressions ba_pose_only_stereo6 uses. */
int ba_right_camera_record(const float *intr_r4, const float *T_lr12,
                           float *camr16);

/* ---- batched planar 3-DoF pose-only (fp32): many problems in one launch --- */
/* B independent Solve_Monocular_Planar3Dof / Solve_Stereo_Planar3Dof problems,
 * laid out and reported as the 6-DoF batch above (ba_po_result, one ba_options,
 * no grid barrier, any B): problem b owns points [offsets[b], offsets[b+1]),
 * intrinsics intr4 + 4b (intr_l4, intr_r4), T_bc12 + 12b, T_wl12 + 12b,
 * T_lr12 + 12b (stereo) and pose T12 + 12b = world_to_current (in/out), rows
 * iters + b*cap and debug poses debug_T12 + 12*b*cap (optional, at most cap
 * each).  A problem of n <= 2048 points gives bit for bit what
 * ba_pose_only_{mono,stereo}3 gives it; larger ones agree to fp32 rounding.
 * T12 is written only where the single call writes it (at least one iteration
 * and no NaN); max_num_iterations <= 0: every pose unchanged, converged, no
 * rows.  Host arrays: B >= 1, offsets[0] == 0, strictly increasing offsets,
 * cap >= 0 and a handle are checked first (else -1, nothing runs); then the
 * records are built on the host, one H2D copy, one launch, one D2H copy and a
 * sync on the handle's stream. */
int ba_pose_only_mono3_batch(ba_handle *h, int B, const int32_t *offsets,
                             const float *X3, const float *uv2,
                             const float *intr4, const float *T_bc12,
                             const float *T_wl12, float *T12, uint8_t *mask,
                             const ba_options *opt, ba_po_iter *iters, int cap,
                             ba_po_result *res, float *debug_T12);
int ba_pose_only_stereo3_batch(ba_handle *h, int B, const int32_t *offsets,
                               const float *X3, const float *uvl2,
                               const float *uvr2, const float *intr_l4,
                               const float *intr_r4, const float *T_bc12,
                               const float *T_lr12, const float *T_wl12,
                               float *T12, uint8_t *mask_l, uint8_t *mask_r,
                               const ba_options *opt, ba_po_iter *iters,
                               int cap, ba_po_result *res, float *debug_T12);
/* The same on DEVICE pointers (offsets and res included), enqueued on
 * hip_stream (NULL = the handle's stream) with no copy and no synchronisation;
 * only the pointers and B are checked on the host.  They take B prepared
 * planar records rec52 (B x 52, from ba_planar_record) instead of T_bc12,
 * T_wl12, T_lr12 and intr_r4, and never READ T12: the prior comes from the
 * record.  T12 is only written, where the single call would write it. */
int ba_pose_only_mono3_batch_device(ba_handle *h, int B, const int32_t *offsets,
                                    const float *X3, const float *uv2,
                                    const float *intr4, const float *rec52,
                                    float *T12, uint8_t *mask,
                                    const ba_options *opt, ba_po_iter *iters,
                                    int cap, ba_po_result *res,
                                    float *debug_T12, void *hip_stream);
int ba_pose_only_stereo3_batch_device(ba_handle *h, int B,
                                      const int32_t *offsets, const float *X3,
                                      const float *uvl2, const float *uvr2,
                                      const float *intr_l4, const float *rec52,
                                      float *T12, uint8_t *mask_l,
                                      uint8_t *mask_r, const ba_options *opt,
                                      ba_po_iter *iters, int cap,
                                      ba_po_result *res, float *debug_T12,
                                      void *hip_stream);
/* Host helper: the per-problem set-up the single planar calls build on the host
 * (the same function):
 *   theta0 (3) | R_cb (9) t_cb (3) | R_bc (9) t_bc (3) | R_rl (9) t_rl (3) |
 *   R_rl*R_cb (9) | right fx fy cx cy (4)  = 52 floats
 * theta0 = (x, y, psi) of the prior pose_b2b1 = T_bc * (T12^-1 * T_wl) * T_bc^-1,
 * psi by the host's atan2.  Mono: T_lr12 = intr_r4 = NULL (stereo fields zero);
 * stereo: both given. */
int ba_planar_record(const float *T_bc12, const float *T_wl12, const float *T12,
                     const float *T_lr12, const float *intr_r4, float *rec52);

/* ---- batched full bundle adjustment: many small windows in one launch ------- */
/* B independent full-BA problems (sliding windows of a few poses and a few hundred
 * landmarks), ONE persistent 256-thread workgroup each: the whole LM loop of Solve
 * (reference :705-1008) — linearisation and damping, Schur complement, reduced solve,
 * back-substitution and trial update, trial cost, model change and trust-region control —
 * runs in fp64 inside one launch, nothing is launched between iterations and no workgroup
 * waits on another (any B: a batch larger than the device holds at once drains).  The
 * arithmetic and every semantic of ba_solve carry over (Huber weights, the last-writer
 * rule for a (landmark, pose) pair observed more than once — observation order inside a
 * problem is significant —, multiplicative damping, the 3x3 inverse with its pivoted
 * fallback, unpivoted Cholesky that zeroes and counts non-positive pivots, the quadratic
 * model on the damped blocks, previous_cost advanced on SKIPPED, "never converged on the
 * last allowed iteration", gauss_newton).  No floating-point atomics, fixed summation
 * order: a problem gives the same bits run to run, alone (B = 1) and at any position of
 * any batch; its sums are ordered differently from the handle path's, so the two agree to
 * rounding, not bit for bit.
 *
 * Limits per problem (ba_batch_info reports them): at most 16 optimisable poses (6N <= 96
 * columns: the reduced system is factored in LDS), at most 64 poses in all (accepted and
 * trial transforms live in LDS), at most 8 cameras; any number of landmarks and
 * observations (per-landmark blocks, pair records and trial points live in a per-problem
 * slice of device scratch allocated at creation).  A problem beyond a limit is NOT solved
 * and reports status 2; every other problem of the batch is solved as if it were absent.
 *
 * The object follows the ba_finalize / ba_update_values split: ba_batch_create plans the
 * structure once (per problem: observations grouped landmark-major with a stable sort,
 * pair lists, last-writer marks) and uploads everything with one copy; values can be
 * replaced and re-solved.  Units and layouts are those of ba_set_*: scaled units, 16-double
 * cameras given as intr4 + T_cj12, 12-double T_jw, problem-LOCAL indices in the
 * observations.  Problem p owns cameras [cam_off[p], cam_off[p+1]), poses, points and
 * observations likewise (B+1 offsets each, starting at 0, never decreasing).  The handle
 * provides the device and the stream; a sharded handle (ba_set_shard world > 1 or an
 * all-reduce hook) or a streamed one is refused, and there is no batched gradient descent.
 * Validation (B >= 1, offsets, indices within their problem, then the handle) happens
 * before anything touches the GPU: -1 and ba_last_error.
 *
 * Lifetime: the batch borrows the handle's device and stream and owns no part of it.  The
 * handle must outlive the batch: ba_batch_destroy first, ba_destroy after; every call on a
 * batch whose handle is gone is undefined. */
typedef struct ba_batch ba_batch;
typedef struct {
  int n_iter, converged, n_rows, status, dropped_pivots;
  /* n_rows = rows logged (rows stored: min(n_rows, cap)); status: 0 = solved, 1 = a pose or
   * point of the problem is not finite on entry (its values are left as given; under LM a
   * non-finite trial cost rejects the step, so values cannot become non-finite later),
   * 2 = over a limit, not solved; dropped_pivots = non-positive pivots the problem's
   * factorisations met (what ba_get_dropped_pivots counts for a handle) */
} ba_batch_result;
int ba_batch_create(ba_batch **out, ba_handle *h, int B, const int32_t *cam_off,
                    const int32_t *pose_off, const int32_t *pt_off,
                    const int64_t *obs_off, const double *cam_intr4,
                    const double *cam_T12, const double *pose_T12,
                    const uint8_t *pose_fixed, const double *pt_X3,
                    const uint8_t *pt_fixed, const int32_t *obs_cam,
                    const int32_t *obs_pose, const int32_t *obs_pt,
                    const double *obs_uv2);
void ba_batch_destroy(ba_batch *b);
/* One ba_options for the whole batch; problem p gets rows + p*cap (rows may be NULL).
 * max_num_iterations <= 0: nothing changes, converged, no rows.  One launch and one
 * synchronisation on the handle's stream.  The solved values stay in the object: a
 * following ba_batch_solve starts from them.  Returns 0 when every problem was processed,
 * whatever its status.
 * With a prior set (ba_batch_set_prior): the prior of a problem is one more factor of its
 * LM loop.  With g = b - H delta at the accepted poses, H_jj joins A_j and g_j joins a_j
 * before damping (the prior's diagonal is damped by 1 + lambda like the rest of A_j), the
 * off-diagonal blocks H_jk join S_jk undamped, the quadratic model gains the cross term
 * 2 sum_{j>k} x_j^T H_jk x_k, and the initial and every trial cost gain the prior's residual
 * norm sqrt(max(0, delta^T H delta - 2 b^T delta + c)).  n_obs (average error) and the block
 * count of the average step are unchanged: a prior is neither an observation nor a
 * parameter block.
 * With relative-pose factors set (ba_batch_set_relative): their blocks are rebuilt from the
 * accepted poses at every linearisation and join A_j, a_j, S_jk, the model and the costs the
 * same way; see there. */
int ba_batch_solve(ba_batch *b, const ba_options *opt, ba_iter_info *rows, int cap,
                   ba_batch_result *res);
/* Covariance blocks of EVERY problem of the batch at the values the object holds (after
 * ba_batch_solve: the solution), one launch and one synchronisation on the handle's stream.
 * Per problem the semantics are those of ba_covariance: linearised with lambda = 0 and the
 * given Huber threshold (last-writer rule of the cross block, the 3x3 inverse with its
 * fallback), S formed and factored unpivoted in LDS, S^-1 = L^-T L^-1 built in place by
 * block triangular inversion (fp64 MFMA), then
 *   cov_pose36  36 per pose of the batch, concatenated user order: [S^-1]_jj, row-major 6x6;
 *   cov_pt9     9 per point of the batch, concatenated user order (NULL: skipped):
 *               Cinv_i + Cinv_i W_i^T Sigma_P(i) W_i Cinv_i, Sigma_P(i) = ALL blocks of S^-1,
 *               off-diagonal ones included, among the poses paired with landmark i.
 * Scaled units, pose tangent xi = [v; omega] of T_jw <- exp(xi) T_jw.  Blocks of fixed poses
 * and fixed points are exactly zero, and so is the block of a never-observed landmark.
 * Every block is symmetric to the bit.  res[p].status follows ba_batch_result (0 = done,
 * 1 = a non-finite value on entry, 2 = over a limit; for 1 and 2 every block of the problem
 * is zero and the other problems are unaffected); res[p].dropped_pivots > 0 tells that S was
 * singular at lambda = 0 (no fixed pose, for example) and the blocks meaningless.
 * Nothing a later call can see changes: poses, points and the bits of a following
 * ba_batch_solve; the per-landmark scratch is overwritten, which ba_batch_solve rebuilds.
 * No floating-point atomics, fixed summation order per problem: the same bits run to run,
 * alone and at any position of any batch, at any image width.  b, cov_pose36 and res are
 * checked for NULL before anything touches the GPU: -1 and ba_last_error.
 * With a prior set (ba_batch_set_prior): S includes the prior's H (lambda = 0) before it is
 * factored, so the blocks are the covariance given the window AND its past.
 * With relative-pose factors set (ba_batch_set_relative): every factor joins S (lambda = 0). */
typedef struct {
  int status, dropped_pivots;
} ba_batch_cov_result;
int ba_batch_covariance(ba_batch *b, double huber, double *cov_pose36, double *cov_pt9,
                        ba_batch_cov_result *res);
/* Marginalisation prior of EVERY problem of the batch at the values the object holds: the
 * Gaussian left on the kept poses when the marked poses, and the landmarks they anchor,
 * leave the window.  One launch and one synchronisation on the handle's stream.
 *   marg_pose   one byte per pose of the batch, concatenated user order: non-zero = marked;
 *   L           the optimisable landmarks with at least one observation from a marked pose
 *               (a marked FIXED pose owns no columns but still selects its landmarks);
 *   factors     every observation (any pose, any camera) of a landmark in L, nothing else;
 *   kept set k  the optimisable, unmarked poses in ascending user order, K of them;
 *   m           the marked optimisable poses.
 * Linearised as ba_batch_covariance does (lambda = 0, the given Huber threshold, last-writer
 * rule, the 3x3 inverse with its fallback, fixed poses feeding C_i and b_i only); with S' and
 * r' the reduced camera system of those factors over the optimisable poses,
 *   H = S'_kk - S'_km S'_mm^-1 S'_mk        b = r'_k - S'_km S'_mm^-1 r'_m,
 * formed in LDS by a partial unpivoted Cholesky (fp64 MFMA) of the image with the marked
 * columns first.  r' has the solver's sign (a_j = -sum Q^T w r): H delta = b is the
 * Gauss-Newton step of the kept poses and the prior energy is 1/2 delta^T H delta - b^T delta,
 * delta the stacked tangents xi = [v; omega] of T_jw <- exp(xi) T_jw at the held values,
 * scaled units, unit pixel noise.
 *   H      problem p: row-major (6 K_p)^2 at element sum_{q<p} 36 K_q^2, symmetric to the bit;
 *   bvec   problem p: 6 K_p at element 6 sum_{q<p} K_q       (ba_batch_marg_layout gives both);
 *   marg_pt  one byte per point of the batch (NULL: skipped): 1 = in L.
 * The rows and columns of a kept pose that observes no landmark of L are exactly zero.  H is
 * in general singular (without a fixed pose observing L it carries the gauge null space);
 * that is not an error.  res[p]: status as ba_batch_cov_result (1 and 2: the problem's output
 * is zero, n_marg_pt is 0, the other problems are unaffected); dropped_pivots = non-positive
 * pivots met while eliminating the MARKED columns (> 0: S'_mm was singular, the prior is
 * meaningless); n_kept = K; n_marg_pose = marked optimisable poses; n_marg_pt = |L|.  A problem
 * with no marked pose gives H = 0, b = 0, status 0; one with every optimisable pose marked
 * (K = 0) has no output, status 0.  Nothing a later call can see changes: poses, points, the
 * bits of a following ba_batch_solve or ba_batch_covariance; the per-landmark scratch is
 * overwritten.  No floating-point atomics, fixed summation order per problem: the same bits
 * run to run, alone and at any position of any batch, at any image width (32, 64, 96 or 112
 * columns, chosen from the widest problem: 16 ceil(6 m / 16) + 6 K).  b, marg_pose, res, and
 * H and bvec unless every K_p = 0, are checked for NULL before anything touches the GPU: -1
 * and ba_last_error.
 * With a prior set (ba_batch_set_prior): the whole prior of a problem, linearised at the held
 * values (H, g = b - H delta), joins the factors before the partial Cholesky, whichever of its
 * poses are marked or kept, so priors chain from window to window.  The output b is then at
 * the held values, which are the T_lin of the next prior.  The rows of a kept pose that
 * touches neither L nor the prior stay exactly zero; the layout and the plan are unchanged.
 * With relative-pose factors set (ba_batch_set_relative): a factor joins exactly when at least
 * one of its two poses is marked (see there); S'_mm may then be well conditioned where it was
 * singular.  The rows of a kept pose that touches neither L, the prior nor a joining factor
 * stay exactly zero. */
typedef struct {
  int status, dropped_pivots, n_kept, n_marg_pose, n_marg_pt;
} ba_batch_marg_result;
int ba_batch_marginalize(ba_batch *b, double huber, const uint8_t *marg_pose, double *H,
                         double *bvec, uint8_t *marg_pt, ba_batch_marg_result *res);
/* Host-only: element offsets of every problem's H and bvec for this marking (B+1 each). */
int ba_batch_marg_layout(ba_batch *b, const uint8_t *marg_pose, int64_t *H_off,
                         int64_t *b_off);
/* Host-only (no GPU): the kept poses (ascending user index, up to n_pose entries) and the
 * landmark set L (one byte per point) of ONE problem under a marking.  kept_pose and marg_pt
 * may be NULL.  Returns K, or -1. */
int ba_batch_marg_plan_problem(int n_pose, const uint8_t *pose_fixed,
                               const uint8_t *marg_pose, int n_pt, const uint8_t *pt_fixed,
                               int64_t n_obs, const int32_t *obs_pose,
                               const int32_t *obs_pt, int32_t *kept_pose, uint8_t *marg_pt);
/* One pose prior per problem: the Gaussian 1/2 delta^T H delta - b^T delta (+ c / 2) that
 * ba_batch_marginalize returns, taken back in as one more factor of ba_batch_solve,
 * ba_batch_covariance and ba_batch_marginalize.  The prior of problem p acts on
 * K_p = prior_off[p+1] - prior_off[p] of its OPTIMISABLE poses:
 *   prior_pose  problem-local user indices, strictly ascending per problem (the order of the
 *               kept set of ba_batch_marginalize);
 *   T_lin12     12 per prior pose, layout of ba_set_poses: the values at which H and b were formed;
 *   H           problem p: row-major (6 K_p)^2 at element sum_{q<p} 36 K_q^2; only the lower
 *               triangle (row >= column) is ever read;
 *   bvec        problem p: 6 K_p at element 6 sum_{q<p} K_q;
 *   c           one per problem, >= 0 (NULL: zeros): the squared residual of the eliminated
 *               factors at the linearisation point.  With c = b^T H^+ b the prior's cost term is
 *               zero at the prior's own minimum; with c = 0 wherever its energy is not positive.
 * Scaled units and the conventions of ba_batch_marginalize: tangent xi = [v; omega] of
 * T_jw <- exp(xi) T_jw, the solver's sign of b, unit pixel noise.  The tangent of pose j is
 * delta_j = se3_log(T_j T_lin,j^-1), the inverse of the solver's se3 exponential; it is defined
 * for a rotation angle below pi and the caller keeps delta small.  The derivative of delta with
 * respect to the update is taken as the identity: first order, exact at delta = 0, the usual
 * choice of a fixed-lag smoother (no right-Jacobian correction, no first-estimate Jacobians).
 * The arrays are copied to the device once; prior_off == NULL clears the prior.  A batch
 * without a prior, and a problem with K_p = 0 whatever its neighbours hold, computes exactly
 * what it computed before: same results, same bits.  One writer per element, fixed summation
 * order, no floating-point atomics: a problem with a prior gives the same bits run to run,
 * alone and at any position of any batch.  A prior given to a problem whose status is 2 is
 * accepted and ignored.  Validation happens before anything touches the GPU (-1 and
 * ba_last_error): offsets start at 0 and never decrease; indices in range, strictly ascending
 * and optimisable; every value finite; c >= 0.  A call refused by the validation changes
 * nothing: the prior set before it stays in effect.  A call that fails later (device
 * allocation, upload) leaves the batch without a prior. */
int ba_batch_set_prior(ba_batch *b, const int32_t *prior_off /* B+1 */, const int32_t *prior_pose,
                       const double *T_lin12, const double *H, const double *bvec,
                       const double *c /* B, NULL = zeros */);
/* Host-only (no GPU): the validation of ba_batch_set_prior for a batch described by pose_off
 * (B+1) and pose_fixed (NULL: none fixed).  0, or -1 and ba_last_error. */
int ba_batch_prior_check(int B, const int32_t *pose_off, const uint8_t *pose_fixed,
                         const int32_t *prior_off, const int32_t *prior_pose,
                         const double *T_lin12, const double *H, const double *bvec,
                         const double *c);
/* out4 = { problems with a prior in effect, their prior poses in all (total K), device bytes
 * of the priors, 0 } */
int ba_batch_prior_info(ba_batch *b, int64_t out4[4]);
/* Relative-pose factors between poses of a problem: odometry between keyframes, a loop closure
 * between two keyframes that share no landmark, the pose part of a pre-integrated inertial
 * delta.  They are more factors of ba_batch_solve, ba_batch_covariance and
 * ba_batch_marginalize, next to the reprojections and the prior.  Problem p carries the
 * factors rel_off[p] .. rel_off[p+1] - 1; several may name the same pair (summed in input
 * order).  Factor f:
 *   rel_j, rel_k  two DISTINCT poses of its problem, problem-local user indices; at least one
 *                 of them optimisable.  A fixed pose receives nothing: the factor is then a
 *                 unary factor on the other pose;
 *   Z12           12 per factor, layout of ba_set_poses: the measurement of T_j T_k^-1;
 *   Omega36       36 per factor, row-major 6x6 information matrix; only the lower triangle
 *                 (row >= column) is ever read.
 * Scaled units and the conventions of ba_batch_set_prior: T = T_jw, tangent xi = [v; omega] of
 * T <- exp(xi) T, unit pixel noise.  Residual r = se3_log(T_j T_k^-1 Z^-1): the prior's delta
 * with T_lin = Z T_k.  Jacobians, first order (exact at r = 0, no left-Jacobian correction:
 * the approximation the prior makes): dr/dxi_j = I, dr/dxi_k = -Ad(T_j T_k^-1), where for
 * T = (R, t) Ad = [[R, [t]x R], [0, R]].  With the solver's sign a = -J^T Omega r:
 *   A_j += Omega,  A_k += Ad^T Omega Ad,  S_jk += -Omega Ad,  a_j += -Omega r,  a_k += Ad^T Omega r.
 * The blocks depend on the poses and are rebuilt at every linearisation.  The diagonal
 * contributions join A_j before the damping (their diagonal is multiplied by 1 + lambda with
 * the rest of A_j), the off-diagonal block joins S undamped, the quadratic model gains
 * 2 x_j^T S_jk x_k.  Every cost (initial and trial) gains sqrt(max(0, r^T Omega r)) per
 * factor: one residual, its norm added as an observation's is; n_obs and the block count of
 * the average step do not change.  There is NO robust weight on relative factors: the Huber
 * threshold acts on reprojections only.  Mind the weights in an LM run: the controller compares a
 * difference of residual NORMS, which grows like sqrt(w) with a factor's weight w, with the
 * quadratic model, which grows like w; one factor some 1e6 times heavier than the reprojection
 * blocks makes the gain ratio about 1e-2 for a perfect step, and every step is rejected.  Scale
 * Omega to the problem, or run such a batch in Gauss-Newton mode.
 * ba_batch_marginalize: a factor joins exactly when at least one of its two poses is marked
 * (optimisable or fixed): it leaves the window with that pose, linearised at the held values,
 * its blocks in S' and r' before the partial factorisation.  A factor between two unmarked
 * poses does not join: the caller carries it into the next window
 * (ba_batch_relative_marg_plan).  Relative factors select no landmarks.  The rows and columns
 * of a kept pose that touches L, the prior or a joining factor are non-zero, those of every
 * other kept pose stay exactly zero.
 * The arrays are copied to the device once, with a scratch of 1008 bytes per factor;
 * rel_off == NULL clears the factors; they survive ba_batch_update_values.  There is no limit
 * on the number of factors of a problem.  A batch without factors, and a problem without
 * factors whatever its neighbours hold, computes exactly what it computed before: same
 * results, same bits.  One writer per element, fixed summation order, no floating-point
 * atomics: the same bits run to run, alone and at any position of any batch.  Factors given
 * to a problem whose status is 2 are accepted and ignored.  Validation happens before anything
 * touches the GPU (-1 and ba_last_error, naming the problem and the factor): offsets start at
 * 0 and never decrease; indices in range; j != k; not both fixed; every value finite.  A call
 * refused by the validation changes nothing: the factors set before it stay in effect.  A
 * call that fails later (device allocation, upload) leaves the batch without factors. */
int ba_batch_set_relative(ba_batch *b, const int32_t *rel_off /* B+1 */, const int32_t *rel_j,
                          const int32_t *rel_k, const double *Z12, const double *Omega36);
/* Host-only (no GPU): the validation of ba_batch_set_relative for a batch described by
 * pose_off (B+1) and pose_fixed (NULL: none fixed).  0, or -1 and ba_last_error. */
int ba_batch_relative_check(int B, const int32_t *pose_off, const uint8_t *pose_fixed,
                            const int32_t *rel_off, const int32_t *rel_j, const int32_t *rel_k,
                            const double *Z12, const double *Omega36);
/* out4 = { problems with factors in effect, factors in effect, device bytes of the factor
 * records plus their scratch, 0 } */
int ba_batch_relative_info(ba_batch *b, int64_t out4[4]);
/* Host-only: rel_leaves[f] = 1, one byte per factor given to ba_batch_set_relative in input
 * order, where factor f joins ba_batch_marginalize under this marking and leaves with the
 * marked poses; 0 where the caller carries it into the next window (and for the ignored
 * factors of a problem whose status is 2). */
int ba_batch_relative_marg_plan(ba_batch *b, const uint8_t *marg_pose, uint8_t *rel_leaves);
/* new values for the same structure, concatenated user order; NULL = keep */
int ba_batch_update_values(ba_batch *b, const double *T_jw12, const double *X3);
int ba_batch_get_poses(ba_batch *b, double *T_jw12);
int ba_batch_get_points(ba_batch *b, double *X3);
/* out8 = { device scratch bytes of the largest problem, LDS bytes of a workgroup, limit
 * of optimisable poses, of poses, of cameras per problem, columns of the LDS image chosen
 * for this batch (32, 64 or 96), device bytes of the whole object, B } */
int ba_batch_info(ba_batch *b, int64_t out8[8]);
/* bytes[p], p < B = device scratch bytes of problem p: the blocks C, b, Cinv, Cinv*b of its
 * optimisable landmarks, the W records of its pairs and its trial points */
int ba_batch_scratch_bytes(ba_batch *b, int64_t *bytes);
/* Host-only (no GPU): the structure ba_batch_create plans for ONE problem.  order[t] =
 * input index of the t-th observation of the landmark-major list (stable), obs_pair[t] =
 * its pair or -1 (pose or point fixed), last_writer[t] = 1 where its cross block survives;
 * pair_lm / pair_pose = optimisable landmark / pose of every pair.  Any output may be NULL.
 * Returns the number of pairs, or -1. */
int ba_batch_plan_problem(int n_pose, const uint8_t *pose_fixed, int n_pt,
                          const uint8_t *pt_fixed, int64_t n_obs,
                          const int32_t *obs_pose, const int32_t *obs_pt,
                          int32_t *order, int32_t *obs_pair, uint8_t *last_writer,
                          int32_t *pair_lm, int32_t *pair_pose);

/* ---- batched full BA: observation report, mask and in-stream outlier cull ------ */
/* Observations are addressed in USER order throughout: the concatenated order of the arrays
 * given to ba_batch_create (observation k of problem p at obs_off[p] + k), never the planned
 * landmark-major order.  Units are those of obs_uv and of the points as given.
 *
 * ba_batch_obs_report: every observation of the batch at the values the object holds, one
 * launch (one thread per observation, no atomics) and one synchronisation:
 *   r2     two doubles per observation: r0, r1 as the solve defines them (projection - uv);
 *   e2     r0^2 + r1^2;
 *   w      the solve's Huber weight for the given threshold: huber / (|r0| + |r1|) where
 *          that sum exceeds huber, else 1;
 *   depth  Xc[2], the depth in the observing camera.
 * Any output may be NULL, not all of them.  Observations that are switched off are reported
 * like the others, and so are problems of status 1 or 2: the values are what the arithmetic
 * gives (non-finite input gives non-finite output).
 *
 * ba_batch_set_obs_mask: obs_on holds one byte per observation, non-zero = on; NULL clears
 * the mask (the original lists are in effect again).  With a mask set, every result of the
 * batch (ba_batch_solve, ba_batch_covariance, ba_batch_marginalize, with or without a prior
 * and relative-pose factors) agrees with the same call on a fresh batch created from the
 * same arrays with the off observations removed, to rounding (a pair of the full structure
 * left without observation adds zeros to the sums): the last-writer rule holds among the on
 * observations of a (landmark, pose) pair, a landmark without on observation has C_i = 0
 * and stays where it is, n_obs of the average error counts the on observations, and the L
 * set of a marginalisation is decided from the on observations.  Nothing is refused for
 * leaving a pose without observations; dropped_pivots reports it.  The mask survives
 * ba_batch_update_values and re-solves.  A problem whose flags are all on gives the bits it
 * gives without a mask.  Mechanism: one launch of k_ba_batch_mask_apply (one workgroup per
 * problem) writes compacted copies of the per-problem observation lists; the solve kernels
 * are the ones a batch without a mask launches.  ba_batch_get_obs_mask returns the mask in
 * effect (all ones without one), also after ba_batch_cull.
 *
 * ba_batch_cull: evaluates the rule at the held values and updates the mask on the device
 * (k_ba_batch_cull, one workgroup per problem, then the mask application).  An observation
 * that is on is switched off iff !(e2 <= e2_max) (a non-finite e2 is culled) or
 * cull_behind != 0 && !(depth > 0).  Observations already off stay off.  Starvation rule: if
 * the rule would leave an optimisable pose of a problem with no on observation although it
 * had one before, that problem's mask is left as it was and it reports starved = 1,
 * n_culled = 0.  A problem of status 1 or 2 is not culled and reports that status (its
 * counts are 0).  A batch that never had a mask gets one by this call.
 *
 * ba_batch_solve_culled: ba_batch_solve with `first`, the cull, ba_batch_solve with `second`,
 * enqueued on the handle's stream with no host synchronisation in between and one at the
 * end.  Stage 2 is an ordinary solve of the masked batch.  Rows: stage 1 writes
 * rows[p*cap + 0 ..], stage 2 from rows[p*cap + first->max_num_iterations] on (res_first[p]
 * .n_rows and res[p].n_rows of them); rows in between are untouched.  rows may be NULL;
 * res_first may be NULL.
 *
 * Refused (-1, ba_last_error, nothing changed, before anything touches the GPU): a null
 * batch, options, result array or cres; e2_max not finite or <= 0; with rows,
 * cap < first->max_num_iterations + second->max_num_iterations; a stage with
 * max_num_iterations <= 0; a report with every output NULL. */
typedef struct { double e2_max; int cull_behind; } ba_cull_options;
typedef struct { int n_on_before, n_culled, starved, status; } ba_batch_cull_result;
int ba_batch_obs_report(ba_batch *b, double huber, double *r2, double *e2, double *w, double *depth);
int ba_batch_set_obs_mask(ba_batch *b, const uint8_t *obs_on);
int ba_batch_get_obs_mask(ba_batch *b, uint8_t *obs_on);
int ba_batch_cull(ba_batch *b, const ba_cull_options *c, ba_batch_cull_result *cres);
int ba_batch_solve_culled(ba_batch *b, const ba_options *first, const ba_options *second,
                          const ba_cull_options *c, ba_iter_info *rows, int cap,
                          ba_batch_result *res_first, ba_batch_result *res,
                          ba_batch_cull_result *cres);
/* Host-only (no GPU): the validation of the cull options. */
int ba_batch_cull_check(const ba_cull_options *c);

/* ---- point-only ("structure-only") solves: every landmark in one launch ------ */
/* The mirror of pose-only: ALL poses are fixed and every landmark is solved on its own.
 * For landmark i with the observations obs_off[i] .. obs_off[i+1]-1 (each a camera, a
 * pose and a pixel, in the caller's order) the result is what ba_solve defines for the
 * problem {all the given cameras and poses, every pose fixed; that one point, optimisable;
 * those observations}: fp64, cost = sum of residual norms, Huber weight on |r_x|+|r_y|,
 * damping diag*(1+lambda), the 3x3 inverse with its fallback, the quadratic model on the
 * damped block, the accept / reject and lambda update of the full solver, previous cost
 * advanced on SKIPPED, "never converged on the last allowed iteration", gauss_newton.
 * In the control step the observation count is the landmark's and the block count is 1.
 * Each landmark has its own lambda, its own decisions and its own stop.
 *
 * triangulate (n_pt bytes, or NULL): a set byte replaces the incoming X by a linear
 * triangulation first: with (R, t) = T_cj o T_jw, x = (u-cx)/fx, y = (v-cy)/fy every
 * observation gives the rows (r1 - x r3).X = -(t1 - x t3), (r2 - y r3).X = -(t2 - y t3);
 * X solves the 3x3 normal equations of all rows (LDL^T in the given order).  The incoming
 * X of such a landmark may be anything, NaN included; the refinement (if
 * max_num_iterations > 0) starts from the triangulated value.
 *
 * Units and layouts are those of ba_set_* (scaled units).  The handle gives the device
 * and the stream only.  One upload, one launch, one download, one synchronisation.
 * rows: n_pt * cap iteration rows (landmark i owns rows[i*cap ..]; n_rows of them are
 * written), or NULL.
 *
 * status: 0 solved.
 *         1 a non-finite value among the landmark's inputs (X when not triangulated, one
 *           of its pixels, cameras or poses): X left as given.
 *         2 no observations: X left as given, no rows (the full solver would log one
 *           SKIPPED row of cost 0 — deliberate deviation).  Decided before status 1.
 *         3 triangulation asked for but degenerate: fewer than two observations, or a
 *           pivot of the normal equations not above 1e-12 of their largest diagonal entry
 *           (a parallax of about 1e-6 rad; exact rank deficiency leaves ~1e-16).  X left
 *           as given, no refinement.
 * n_behind: observations with non-positive depth in their camera at the returned X (0
 * for status 1 and 2).  cost0 / cost: the first previous cost and the accepted cost at
 * the end.  dropped_pivots: iterations whose inverse of the damped block had a diagonal
 * entry that was not positive (the block was not positive definite).
 * max_num_iterations <= 0: triangulation only, where asked; otherwise X unchanged;
 * converged = 1, no rows.
 * One writer per value, fixed summation order per landmark, no atomics: a landmark gives
 * the same bits run to run, alone and at any position of any call (for one team width).
 * Everything is validated on the host before anything touches the GPU (-1 and
 * ba_last_error naming the landmark / observation): n_cam, n_pose, n_pt >= 1, offsets
 * starting at 0 and never decreasing, camera and pose indices in range, non-NULL
 * pointers (triangulate and rows may be NULL), cap >= 0. */
typedef struct {
  int n_iter, converged, n_rows, status, n_behind, dropped_pivots;
  double cost0, cost;
} ba_point_result;
int ba_point_only(ba_handle *h, int n_cam, const double *intr4, const double *T_cj12,
                  int n_pose, const double *T_jw12, int n_pt, const int64_t *obs_off /* n_pt+1 */,
                  const int32_t *obs_cam, const int32_t *obs_pose, const double *obs_uv2,
                  const uint8_t *triangulate /* n_pt or NULL */, double *X3 /* in/out */,
                  const ba_options *opt, ba_iter_info *rows /* n_pt*cap or NULL */, int cap,
                  ba_point_result *res);
/* Host-only (no GPU): the validation of the structure arguments of ba_point_only. */
int ba_point_only_check(int n_cam, int n_pose, int n_pt, const int64_t *obs_off,
                        const int32_t *obs_cam, const int32_t *obs_pose);
/* Lanes per landmark of the kernel: 8 or 16 (two instantiations; the sums of a landmark
 * are associated differently, so the last bits differ between the widths).  width = 0
 * asks; 8 / 16 sets it for the process.  Returns the width in force, or -1.  The default
 * is the width measured faster at 10 observations per landmark. */
int ba_point_only_team(int width);
/* Device time (hipEvents around the launch) of the calling thread's last ba_point_only. */
int ba_point_only_last_ms(double *kernel_ms);

/* ---- pose-graph optimisation ----------------------------------------------
 * Levenberg-Marquardt over relative-pose factors ALONE: keyframe poses, odometry and
 * loop-closure edges, no camera, landmark or observation.  The reference project has no
 * counterpart; this comment is the definition.
 *
 * Inputs: n_pose poses T_jw (12 doubles each, scaled units), their fixed flags (NULL: none
 * fixed) and n_rel factors exactly as ba_set_relative defines them: r_f = se3_log(T_j T_k^-1
 * Z_f^-1), first-order Jacobians I and -Ad(T_j T_k^-1), Omega read from its lower triangle,
 * several factors may name one pair in either orientation, summed in input order.
 *
 * System over the N optimisable poses: chi2(T) = sum_f r_f^T Omega_f r_f (no square root, no
 * sum of norms),
 *   H_jj += Omega,  H_kk += Ad^T Omega Ad,  H_jk += -Omega Ad,  g_j += -Omega r,  g_k += Ad^T Omega r;
 * a fixed pose receives nothing.  Step (H + lambda diag(H)) x = g, trial poses
 * T_j <- se3_exp(x_j) T_j.
 *
 * Gain ratio: pred = g^T x + lambda x^T diag(H) x, rho = (chi2_accepted - chi2_trial) / pred.
 * rho > 0.25 accepts (status 0); otherwise the step is rejected (status 2) and the accepted
 * chi-square stays the comparison value.  rho > 0.5: lambda = max(1e-10, lambda *
 * decrease_ratio_lambda), status 1.  rho <= 0.25: lambda = min(1e10, lambda *
 * increase_ratio_lambda).  gauss_newton = 1: every step accepted, lambda stays at
 * initial_lambda, rho = pred = 0.
 *
 * Stop: the mean over the optimisable poses of |x_j| < threshold_step_size, or |chi2_accepted
 * - chi2_trial| < threshold_cost_change; never in the last allowed iteration.
 * threshold_huber_loss and threshold_outlier_rejection are unused: robust weights are per
 * factor (ba_pgraph_set_robust below), none by default.
 *
 * Rows: cost = accepted chi-square after the iteration, trial_cost, cost_change (0 on a
 * rejection), average_reprojection_error = sqrt(cost / factors), abs_step = the mean step,
 * damping_term = lambda after the update, rho, model_change = pred, iteration_status.
 *
 * The object keeps the structure (lists, the level schedule of the tile Cholesky, the dense
 * image of npad x (npad + nb) doubles) across re-solves, as ba_batch does.  It borrows the
 * handle's device, stream and BA_DENSE_* knobs: ba_pgraph_destroy first, ba_destroy after.
 * The handle needs no problem of its own, and a problem it holds is not touched.
 *
 * Validation happens before anything touches the GPU, with the rules and messages of
 * ba_relative_check (-1 and ba_last_error naming the factor); also refused: n_pose <= 0,
 * n_rel <= 0, a non-finite pose, and an optimisable pose that no factor names (the message
 * names the pose; its diagonal would be zero).  A graph without a fixed pose is NOT refused:
 * the damping holds it, and ba_pgraph_info reports the non-positive pivots.  If the image
 * cannot be allocated the call fails with its size in the message, before any launch.  A
 * refused call changes nothing.
 *
 * One writer per element, fixed summation order, no floating-point atomics: the same bits
 * run to run. */
typedef struct ba_pgraph ba_pgraph;
int ba_pgraph_create(ba_pgraph **out, ba_handle *h, int n_pose, const double *T_jw12,
                     const uint8_t *pose_fixed, int64_t n_rel, const int32_t *rel_j,
                     const int32_t *rel_k, const double *Z12, const double *Omega36);
void ba_pgraph_destroy(ba_pgraph *g);
/* New VALUES for the same structure; NULL = keep.  Validated as at creation. */
int ba_pgraph_update_values(ba_pgraph *g, const double *T_jw12, const double *Z12,
                            const double *Omega36);
/* The whole loop is enqueued for max_num_iterations without a host round trip; one
 * synchronisation at the end.  At most cap rows are written (rows may be NULL); rows beyond
 * *n_iter are untouched.  The solved poses stay in the object.  max_num_iterations <= 0:
 * nothing changes, *n_iter = 0, *converged = 1. */
int ba_pgraph_solve(ba_pgraph *g, const ba_options *opt, ba_iter_info *rows, int cap,
                    int *n_iter, int *converged);
int ba_pgraph_get_poses(ba_pgraph *g, double *T_jw12);
/* chi-square at the poses the object holds */
int ba_pgraph_cost(ba_pgraph *g, double *chi2);
/* The undamped system at the poses the object holds, for tests: H (6N x 6N, row-major, both
 * triangles) and g (6N); optimisable poses in the user's order.  Either may be NULL.  With
 * robust kernels set: the weighted system. */
int ba_pgraph_get_system(ba_pgraph *g, double *H, double *g6N);
/* out8 = { N, factors, coupled blocks, tile order, tiles, levels, bytes of the dense image,
 * non-positive pivots of the last solve } */
int ba_pgraph_info(ba_pgraph *g, int64_t out8[8]);
/* Device time of the last ba_pgraph_solve, from events around the enqueued loop. */
int ba_pgraph_last_ms(ba_pgraph *g, double *ms);
/* Host-only (no GPU): the validation of ba_pgraph_create. */
int ba_pgraph_check(int n_pose, const double *T_jw12, const uint8_t *pose_fixed, int64_t n_rel,
                    const int32_t *rel_j, const int32_t *rel_k, const double *Z12,
                    const double *Omega36);

/* ---- robust kernels on the factors of a pose graph ------------------------
 * Every factor has a kernel kind and a scale c > 0, a Mahalanobis distance.  With
 * s_f = r_f^T Omega_f r_f:
 *
 *   kind              rho(s)                                  w(s) = rho'(s)
 *   0 none            s                                       1
 *   1 Huber           s if s <= c^2, else 2 c sqrt(s) - c^2   1 if s <= c^2, else c / sqrt(s)
 *   2 Cauchy          c^2 log1p(s / c^2)                      1 / (1 + s / c^2)
 *   3 Geman-McClure   c^2 s / (c^2 + s)                       (c^2 / (c^2 + s))^2
 *
 * Geman-McClure is the closed form of switchable constraints with Phi = c^2.  s = 0 gives
 * w = 1 for every kind; nothing divides by s except Huber beyond its knee, where s > c^2 > 0.
 *
 * Cost: the solver's chi-square is sum_f rho_f(s_f): the accepted cost, the trial cost,
 * ba_pgraph_cost and every row field derived from them (cost, trial_cost, cost_change,
 * average_reprojection_error, rho).
 * System: H and g exactly as above with w_f Omega_f in place of Omega_f, w_f taken at the
 * poses of the linearisation, which are the accepted poses; after a rejected step the records
 * and the weights stay.  The weighted Gauss-Newton model has exactly the gradient of
 * sum rho(s), so pred = g^T x + lambda x^T diag(H) x stays the matching model.  There is NO
 * second-order (Triggs) correction: the term 2 rho''(s) (J^T Omega r)(J^T Omega r)^T is left out.
 * Control, stop test, Gauss-Newton mode and the log rows are unchanged.
 *
 * kind == NULL clears every kernel; the scale of a kind-0 factor is ignored (scale may be NULL
 * if every kind is 0).  May be called between solves any number of times without re-planning:
 * shrinking c from solve to solve is the caller's graduated non-convexity.
 * ba_pgraph_update_values keeps the kernels.  A graph with no kernel set, or with all kinds 0,
 * launches exactly the kernels of the section above (k_pg_lin, k_pg_assemble); otherwise their
 * robust instantiations (k_pg_lin_robust, k_pg_assemble_robust) run in their place.
 * Refused (-1, ba_last_error names the factor; nothing changes): a kind outside 0..3, and on a
 * factor whose kind is not 0 a scale that is not finite or <= 0. */
int ba_pgraph_set_robust(ba_pgraph *g, const int32_t *kind /* F or NULL */,
                         const double *scale /* F */);
/* Host-only (no GPU): the validation of ba_pgraph_set_robust. */
int ba_pgraph_robust_check(int64_t n_rel, const int32_t *kind, const double *scale);
/* s_f and w_f of every factor (F doubles each, input order) at the poses the object holds,
 * from one pass like ba_pgraph_cost; a factor without a kernel reports w = 1.  Either output
 * may be NULL.  This is how a caller finds the closures to drop. */
int ba_pgraph_factor_report(ba_pgraph *g, double *s, double *w);

/* ---- covariance blocks of a pose graph and a chi-square gate ---------------
 * How well the poses the object holds are determined, and whether a loop-closure candidate is
 * consistent with them BEFORE it enters the graph (g2o's computeMarginals, GTSAM's Marginals;
 * the robust kernels above act only after a false closure has bent the solve).
 *
 * System: H is exactly what ba_pgraph_get_system returns: lambda = 0, the accepted poses,
 * w_f Omega_f for a factor with a robust kernel, w_f at those poses.  Sigma = H^-1 over the
 * optimisable poses, scaled units, tangent xi = [v; omega] of T <- exp(xi) T; a fixed pose has
 * zero blocks.  The call factorises H with the solve's launches (no level goes to the LDS tail
 * kernel, so the whole factor stays in the image) and reads the blocks off the factor
 * (csrc/ba_graph_kernels.hip, fp64 MFMA, no atomics: the same bits run to run, in any selection
 * and any batch split).
 *   cov_pose36[s]   Sigma_jj of pose pose_sel[s] (6x6 row-major)
 *   cov_cross36[p]  Sigma_jk of the pair (pair_j[p], pair_k[p]); may be NULL
 *   cov_rel36[p]    Sigma_E, the covariance of the relative pose E = T_j T_k^-1, which moves to
 *                   first order by xi_E = xi_j - Ad(E) xi_k (the factor's own Jacobians):
 *                   Sigma_E = Sigma_jj - Sigma_jk Ad^T - Ad Sigma_kj + Ad Sigma_kk Ad^T;
 *                   with j fixed it is Ad Sigma_kk Ad^T, with k fixed Sigma_jj
 * pose_sel: USER indices of optimisable poses, any order, repeats allowed.  Pairs: user
 * indices, the pair rules of ba_relative_check (in range, j != k, not both fixed), repeats and
 * both orientations allowed; every pair is swept on its own.  Either selection may be empty
 * (its outputs then NULL); with both empty the call factorises and writes nothing.
 * dropped_pivots (may be NULL) receives the non-positive pivots THIS call's factorisation met.
 * A graph without a fixed pose is singular at lambda = 0 and the result meaningless:
 * dropped_pivots > 0 is how the caller learns of it.
 *
 * State: the poses, the controller, the robust kernels, ba_pgraph_last_ms and the pivot count
 * of ba_pgraph_info are untouched: a solve after the call gives the bits it gives without.
 * Refused (-1, ba_last_error names the entry, before anything touches the GPU; nothing
 * changes): a null graph, a NULL output for a non-empty selection, a pose_sel entry out of
 * range or naming a fixed pose, a pair that ba_relative_check would refuse as a factor.
 * The right-hand sides (16 per wave: two selected poses, or one pair) go in column batches; the
 * workspace, npad x batch x 8 bytes, is allocated for the call and freed on return. */
int ba_pgraph_covariance(ba_pgraph *g, int n_pose_sel, const int32_t *pose_sel, double *cov_pose36,
                         int64_t n_pair, const int32_t *pair_j, const int32_t *pair_k,
                         double *cov_cross36 /* or NULL */, double *cov_rel36,
                         int64_t *dropped_pivots);
/* The gate.  A candidate (j, k, Z, Omega_z) has the shape of a factor: r = se3_log(E Z^-1),
 * P = Sigma_E + Omega_z^-1 (the innovation covariance) and d2[c] = r^T P^-1 r, to be compared
 * with a chi-square quantile of 6 degrees of freedom (22.46 at 0.999).  Sigma_E is first order
 * and taken at lambda = 0, as above.  Only the lower triangle of Omega_z counts; no robust
 * weight applies to a candidate.  r6 (6 per candidate) and innov36 (= P) may be NULL.  A P
 * with a non-positive pivot yields d2 = NaN.  State, batching and dropped_pivots as above.
 * Refused likewise: what ba_relative_check refuses (same rules, same wording, "candidate" for
 * "factor"), and a candidate whose Omega_z is not positive definite (6x6 Cholesky of the
 * mirrored lower triangle on the host; the message names the candidate). */
int ba_pgraph_gate(ba_pgraph *g, int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k,
                   const double *Z12, const double *Omega36, double *d2, double *r6 /* or NULL */,
                   double *innov36 /* or NULL */, int64_t *dropped_pivots);
/* Host-only (no GPU): the validation of both calls on plain arrays: the fixed mask of the
 * n_pose poses (NULL: none fixed), the selection and pairs of ba_pgraph_covariance, the
 * candidates of ba_pgraph_gate, and the output pointers cov_pose36, cov_rel36 and d2.  0 or -1. */
int ba_pgraph_cov_check(int n_pose, const uint8_t *pose_fixed, int n_pose_sel,
                        const int32_t *pose_sel, const double *cov_pose36, int64_t n_pair,
                        const int32_t *pair_j, const int32_t *pair_k, const double *cov_rel36,
                        int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k,
                        const double *Z12, const double *Omega36, const double *d2);
/* out4 = { columns of one batch on this graph (what fits 256 MiB of workspace, at most 16384;
 * BA_COV_BATCH=<columns> of the borrowed handle overrides), columns per wave (16), batches the
 * last ba_pgraph_covariance / ba_pgraph_gate ran, bytes of the workspace at that width } */
int ba_pgraph_cov_info(ba_pgraph *g, int64_t out4[4]);

/* ---- Sim(3) pose-graph optimisation ----------------------------------------
 * The 7-DoF loop closing of a monocular map: Levenberg-Marquardt over relative-similarity
 * factors ALONE.  A monocular map drifts in scale, and a rigid graph spreads that drift into
 * translation; here every keyframe carries a scale as well.  The reference project has no
 * counterpart; this comment is the definition.
 *
 * Pose: S_jw = (R, t, s), stored as 13 doubles S13 = { R row-major (9), t (3), s }, s > 0,
 * translation in scaled units.  It maps x_j = s R x_w + t; as a matrix [[sR, t], [0, 1]].
 *
 * Tangent: xi = [v; omega; sigma] (7), algebra element [[hat(omega) + sigma I, v], [0, 0]].
 *   sim3_exp(xi) = (exp(hat(omega)), W v, e^sigma),
 *   W = integral_0^1 e^(tau sigma) exp(tau hat(omega)) d tau;
 * sim3_log is its inverse on rotation angles below pi.
 *
 * Update: S_j <- sim3_exp(x_j) S_j, the left perturbation of the SE(3) graph.
 *
 * Factor: (j, k, Z13, Omega49).  Z measures E = S_j S_k^-1; r = sim3_log(E Z^-1); the
 * first-order Jacobians are I on j and -Ad7(E) on k, where for E = (R, t, s)
 *   Ad7(E) = [[sR, hat(t) R, -t], [0, R, 0], [0, 0, 1]].
 * Omega is read from its lower triangle.  Several factors may name one pair in either
 * orientation; they are summed in input order.
 *
 * Cost and system over the N optimisable poses: chi2 = sum_f r_f^T Omega_f r_f,
 *   H_jj += Omega,  H_kk += Ad7^T Omega Ad7,  H_jk += -Omega Ad7,
 *   g_j += -Omega r,  g_k += Ad7^T Omega r,
 * with 7x7 blocks; a fixed pose (all seven components) receives nothing.  Step
 * (H + lambda diag(H)) x = g.
 *
 * Control: step, gain ratio, lambda update, Gauss-Newton mode, stop test and rows are those of
 * ba_pgraph_solve above, word for word; the mean step is the mean of |x_j| over 7 components.
 *
 * The object keeps the structure (lists, level schedule, the dense image of npad x (npad + nb)
 * doubles with seven columns per pose: 4 poses per tile of order 32, 9 per tile of order 64)
 * across re-solves and borrows the handle's device, stream and BA_DENSE_* knobs:
 * ba_sim3_destroy first, ba_destroy after.  A problem or an SE(3) graph on the same handle is
 * not touched.
 *
 * Validation happens before anything touches the GPU, with the rules and messages of
 * ba_pgraph_check ("S_jw" for "T_jw"); also refused: a scale of a pose or of Z that is not
 * finite or not positive, and a rotation part of a pose or of Z that is not finite (the
 * message names the pose or the factor).  If the image cannot be allocated the call fails with
 * its size in the message, before any launch.  A refused call changes nothing.
 *
 * One writer per element, fixed summation order, no floating-point atomics: the same bits run
 * to run.  Robust kernels, covariance blocks and the 7-DoF gate: the two sections below. */
typedef struct ba_sim3 ba_sim3;
int ba_sim3_create(ba_sim3 **out, ba_handle *h, int n_pose, const double *S13,
                   const uint8_t *pose_fixed, int64_t n_rel, const int32_t *rel_j,
                   const int32_t *rel_k, const double *Z13, const double *Omega49);
void ba_sim3_destroy(ba_sim3 *g);
/* New VALUES for the same structure; NULL = keep.  Validated as at creation. */
int ba_sim3_update_values(ba_sim3 *g, const double *S13, const double *Z13, const double *Omega49);
/* As ba_pgraph_solve: the whole loop is enqueued, one synchronisation at the end; at most cap
 * rows are written, rows beyond *n_iter are untouched; the solved poses stay in the object. */
int ba_sim3_solve(ba_sim3 *g, const ba_options *opt, ba_iter_info *rows, int cap, int *n_iter,
                  int *converged);
int ba_sim3_get_poses(ba_sim3 *g, double *S13);
/* chi-square at the poses the object holds */
int ba_sim3_cost(ba_sim3 *g, double *chi2);
/* The undamped system at the poses the object holds, for tests: H (7N x 7N, row-major, both
 * triangles) and g (7N); optimisable poses in the user's order.  Either may be NULL. */
int ba_sim3_get_system(ba_sim3 *g, double *H, double *g7N);
/* s_f = r_f^T Omega_f r_f of every factor at the poses the object holds (n_rel doubles) */
int ba_sim3_factor_report(ba_sim3 *g, double *s);
/* out9 = { N, factors, coupled blocks, tile order, tiles, levels, bytes of the dense image,
 * non-positive pivots of the last solve, factors per k_s3_lin workgroup } */
int ba_sim3_info(ba_sim3 *g, int64_t out9[9]);
/* Device time of the last ba_sim3_solve, from events around the enqueued loop. */
int ba_sim3_last_ms(ba_sim3 *g, double *ms);
/* Host-only (no GPU): the validation of ba_sim3_create. */
int ba_sim3_check(int n_pose, const double *S13, const uint8_t *pose_fixed, int64_t n_rel,
                  const int32_t *rel_j, const int32_t *rel_k, const double *Z13,
                  const double *Omega49);
/* Host-only (no GPU): the functions the kernels call (csrc/ba_sim3_fn.h), for tests of the
 * arithmetic.  xi7 = [v; omega; sigma]; Ad49 row-major. */
void ba_sim3_exp(const double *xi7, double *S13);
void ba_sim3_log(const double *S13, double *xi7);
void ba_sim3_adjoint(const double *S13, double *Ad49);

/* ---- robust kernels on the factors of a Sim(3) graph -----------------------
 * The block of ba_pgraph_set_robust above, word for word, at width 7: the same kinds 0..3 with
 * the same rho and w table, s_f = r_f^T Omega_f r_f with r of 7 components.  Chi-square is
 * sum_f rho_f(s_f) in the accepted cost, the trial cost, ba_sim3_cost and every row field derived
 * from them.  H and g use w_f Omega_f, w_f taken at the accepted poses; after a rejected step the
 * records and the weights stay.  No second-order (Triggs) term.  Control, stop test,
 * Gauss-Newton mode and rows are unchanged.
 *
 * kind == NULL clears every kernel; the scale of a kind-0 factor is ignored (scale may be NULL
 * if every kind is 0).  May be called between solves any number of times without re-planning.
 * ba_sim3_update_values keeps the kernels.  A graph with no kernel set, or with all kinds 0,
 * launches exactly k_s3_lin and k_s3_assemble; otherwise k_s3_lin_robust and
 * k_s3_assemble_robust run in their place.  Refused (-1, ba_last_error names the factor; nothing
 * changes): what ba_pgraph_set_robust refuses, in its wording. */
int ba_sim3_set_robust(ba_sim3 *g, const int32_t *kind /* F or NULL */, const double *scale /* F */);
/* Host-only (no GPU): the validation of ba_sim3_set_robust. */
int ba_sim3_robust_check(int64_t n_rel, const int32_t *kind, const double *scale);
/* s_f and w_f of every factor (F doubles each, input order) at the poses the object holds, from
 * one pass like ba_sim3_cost; a factor without a kernel reports w = 1.  Either output may be
 * NULL.  ba_sim3_factor_report above keeps its signature and its bits. */
int ba_sim3_factor_weights(ba_sim3 *g, double *s, double *w);

/* ---- covariance blocks of a Sim(3) graph and the 7-DoF chi-square gate ------
 * The block of ba_pgraph_covariance / ba_pgraph_gate above at width 7.
 *
 * System: H is exactly what ba_sim3_get_system returns: lambda = 0, the poses the object holds,
 * w_f Omega_f where a robust kernel is set.  Sigma = H^-1 over the optimisable poses, scaled
 * units, tangent xi = [v; omega; sigma] of S <- sim3_exp(xi) S; a fixed pose has zero blocks.
 *   cov_pose49[s]   Sigma_jj of pose pose_sel[s] (7x7 row-major)
 *   cov_cross49[p]  Sigma_jk of the pair (pair_j[p], pair_k[p]); may be NULL
 *   cov_rel49[p]    Sigma_E = Sigma_jj - Sigma_jk Ad7^T - Ad7 Sigma_kj + Ad7 Sigma_kk Ad7^T, the
 *                   covariance of E = S_j S_k^-1 with Ad7 = Ad7(E); with j fixed it is
 *                   Ad7 Sigma_kk Ad7^T, with k fixed Sigma_jj
 * Selections, repeats, both orientations, empty selections, dropped_pivots, batching and the
 * treatment of the object's state (the poses, the controller, the robust kernels,
 * ba_sim3_last_ms and the pivot count of ba_sim3_info are untouched) are those of
 * ba_pgraph_covariance.  The kernels are csrc/ba_graph_kernels.hip: fp64 MFMA sweep, no atomics, the
 * same bits run to run, in any selection and any batch split. */
int ba_sim3_covariance(ba_sim3 *g, int n_pose_sel, const int32_t *pose_sel, double *cov_pose49,
                       int64_t n_pair, const int32_t *pair_j, const int32_t *pair_k,
                       double *cov_cross49 /* or NULL */, double *cov_rel49,
                       int64_t *dropped_pivots);
/* The gate.  A candidate (j, k, Z13, Omega49) has the shape of a factor: r = sim3_log(E Z^-1),
 * P = Sigma_E + Omega_z^-1 and d2[c] = r^T P^-1 r, to be compared with a chi-square quantile of
 * 7 degrees of freedom (24.32 at 0.999).  Only the lower triangle of Omega_z counts; no robust
 * weight applies to a candidate.  r7 (7 per candidate) and innov49 (= P) may be NULL.  A P with
 * a non-positive pivot yields d2 = NaN.  Refused before anything touches the GPU: what
 * ba_pgraph_gate refuses ("candidate" for "factor"), a candidate whose scale is not finite or
 * not positive or whose rotation is not finite (the wording of ba_sim3_check), and a candidate
 * whose Omega_z is not positive definite (7x7 Cholesky of the mirrored lower triangle on the
 * host; the message names the candidate). */
int ba_sim3_gate(ba_sim3 *g, int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k,
                 const double *Z13, const double *Omega49, double *d2, double *r7 /* or NULL */,
                 double *innov49 /* or NULL */, int64_t *dropped_pivots);
/* Host-only (no GPU): the validation of both calls on plain arrays, as ba_pgraph_cov_check. */
int ba_sim3_cov_check(int n_pose, const uint8_t *pose_fixed, int n_pose_sel,
                      const int32_t *pose_sel, const double *cov_pose49, int64_t n_pair,
                      const int32_t *pair_j, const int32_t *pair_k, const double *cov_rel49,
                      int64_t n_cand, const int32_t *cand_j, const int32_t *cand_k,
                      const double *Z13, const double *Omega49, const double *d2);
/* out4 as ba_pgraph_cov_info: { columns of one batch on this graph, columns per wave (16),
 * batches the last ba_sim3_covariance / ba_sim3_gate ran, bytes of the workspace at that width } */
int ba_sim3_cov_info(ba_sim3 *g, int64_t out4[4]);

#ifdef __cplusplus
}
#endif
#endif /* BA_HIP_H_ */
