// FullBundleAdjustmentSolver — C++ host facade over the HIP C ABI
// (include/ba_hip.h).  Same namespace, class name, typedef names and method
// signatures as the reference (core/full_bundle_adjustment_solver.h:34-146),
// so a caller such as reference test/test_ba.cpp compiles against this header
// unchanged.  What the facade does on the host is exactly what the
// reference's Add* methods do (pointer -> index maps, 0.01 scaling, pose
// inversion, write-back); the whole LM loop runs on the GPU.
#ifndef BA_FACADE_FULL_BUNDLE_ADJUSTMENT_SOLVER_H_
#define BA_FACADE_FULL_BUNDLE_ADJUSTMENT_SOLVER_H_

#include <cstdint>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "core/solver_option_and_summary.h"
#include "eigen3/Eigen/Dense"
#include "utility/timer.h"

struct ba_handle;  // include/ba_hip.h
struct ba_batch;

namespace visual_navigation {
namespace analytic_solver {

using _BA_Numeric = double;
using _BA_Index = int;
using _BA_Size_t = int;
using _BA_Mat33 = Eigen::Matrix<_BA_Numeric, 3, 3>;
using _BA_Mat66 = Eigen::Matrix<_BA_Numeric, 6, 6>;
using _BA_Vec2 = Eigen::Matrix<_BA_Numeric, 2, 1>;
using _BA_Vec3 = Eigen::Matrix<_BA_Numeric, 3, 1>;
using _BA_Vec6 = Eigen::Matrix<_BA_Numeric, 6, 1>;
using _BA_Pixel = Eigen::Matrix<_BA_Numeric, 2, 1>;
using _BA_Point = Eigen::Matrix<_BA_Numeric, 3, 1>;
using _BA_Rotation3 = Eigen::Matrix<_BA_Numeric, 3, 3>;
using _BA_Position3 = Eigen::Matrix<_BA_Numeric, 3, 1>;
using _BA_Pose = Eigen::Transform<_BA_Numeric, 3, 1>;
using _BA_PixelVec = std::vector<_BA_Pixel>;
using _BA_PointVec = std::vector<_BA_Point>;
using _BA_IndexVec = std::vector<_BA_Index>;

struct _BA_Camera {
  _BA_Camera() {}
  _BA_Camera(const _BA_Camera &camera)
      : fx(camera.fx), fy(camera.fy), cx(camera.cx), cy(camera.cy), pose_this_to_cam0(camera.pose_this_to_cam0) {}
  _BA_Camera &operator=(const _BA_Camera &camera) = default;
  _BA_Numeric fx{0.0};
  _BA_Numeric fy{0.0};
  _BA_Numeric cx{0.0};
  _BA_Numeric cy{0.0};
  _BA_Pose pose_this_to_cam0;  // body -> this camera
};

class FullBundleAdjustmentSolver {
 public:
  FullBundleAdjustmentSolver();
  ~FullBundleAdjustmentSolver();
  FullBundleAdjustmentSolver(const FullBundleAdjustmentSolver &) = delete;
  FullBundleAdjustmentSolver &operator=(const FullBundleAdjustmentSolver &) = delete;

  void Reset();

  void AddCamera(const _BA_Index camera_index, const _BA_Camera &camera);
  void AddPose(_BA_Pose *original_pose);
  void AddPoint(_BA_Point *original_point);
  void AddObservation(const _BA_Index index_camera, _BA_Pose *related_pose, _BA_Point *related_point,
                      const _BA_Pixel &pixel);

  void MakePoseFixed(_BA_Pose *original_pose_to_be_fixed);
  void MakePointFixed(_BA_Point *original_point_to_be_fixed);

  // Private in the reference (called inside Solve); public and idempotent
  // here, as the reference README lists it in the usage sequence.
  void FinalizeParameters();

  bool Solve(Options options, Summary *summary = nullptr);

  // (new; the reference has no counterpart) Pose-graph optimisation: Levenberg-Marquardt over
  // the factors of AddRelativePose ALONE, on the registered poses with their fixed flags
  // (ba_pgraph_* of include/ba_hip.h: chi-square LM, the definition is there).  Needs no
  // camera, point, observation or FinalizeParameters; the solver's current values are used and
  // the solved poses become them, written back through the caller's pointers as Solve writes
  // them.  The rows of `summary` are those of ba_pgraph_solve.  A finalized problem of the same
  // solver takes the new poses with ReloadParameterValues.  Throws std::runtime_error without
  // poses or factors, and on every refusal of ba_pgraph_create.  A factor that carries a robust
  // kernel (RelativePose::robust_kind) is solved with it (ba_pgraph_set_robust).
  bool SolvePoseGraph(Options options, Summary *summary = nullptr);
  // (new) The factor report of the last SolvePoseGraph at the solved poses, one entry per
  // factor in the order of AddRelativePose (ba_pgraph_factor_report): s = r^T information r in
  // the caller's units, the Mahalanobis distance squared that a robust scale is compared with,
  // and the robust weight w (1 for a factor without a kernel).  A closure with a small w is
  // the one to drop.  Either output may be null.  Throws std::runtime_error before the first
  // SolvePoseGraph.
  void GetRelativeWeights(std::vector<double> *s, std::vector<double> *w) const;

  // (new) A relative-similarity factor between two registered poses for SolveSim3Graph, the
  // 7-DoF loop closing of a monocular map (ba_sim3_* of include/ba_hip.h; the definition is
  // there).  measurement: the row-major 4x4 similarity [[sR, t], [0, 1]], the measured
  // inverse(*pose_j) * (*pose_k) in the convention and units of AddPose (s = 1: a rigid edge).
  // information: the row-major 7x7 of the tangent [v; omega; sigma] in the caller's units,
  // converted for sigma_pixel as RelativePose::information is (sigma, like omega, has no unit);
  // only its lower triangle is read.
  struct RelativeSim3 {
    _BA_Pose *pose_j{nullptr};
    _BA_Pose *pose_k{nullptr};
    double measurement[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    double information[49] = {0.0};
    // (new) a robust kernel for SolveSim3Graph, as RelativePose::robust_kind / robust_scale:
    // 0 none (the default; robust_scale is then unread), 1 Huber, 2 Cauchy, 3 Geman-McClure;
    // robust_scale is the Mahalanobis distance c > 0 against `information` as given, in the
    // caller's units with sigma_pixel
    int robust_kind{0};
    double robust_scale{0.0};
  };
  // (new) May be called at any time; Reset drops the factors.  Solve, SolveBatch,
  // ComputeCovariance and SolvePoseGraph never see them, and SolveSim3Graph sees no factor of
  // AddRelativePose.  Throws std::runtime_error on a pose that was never registered.
  void AddRelativeSim3(const RelativeSim3 &factor, double sigma_pixel = 1.0);
  // (new) Sim(3) pose-graph optimisation over the factors of AddRelativeSim3 ALONE.  Every
  // registered pose starts as the similarity (R, t, s = 1) of its rigid pose; the rows of
  // `summary` are those of ba_sim3_solve.  Each pose is written back RIGID, T_jw = [R, t / s];
  // *scales (may be null) receives s per registered pose (1 for a fixed pose).
  // point_anchors (null: no point moves): one entry per registered point in registration order,
  // the registration index of a pose or -1.  An anchored, non-fixed point moves to
  // S_new,a^-1 (T_old,a X), so that its projection into its anchor keyframe is unchanged (on the
  // host).  The solver's own copies follow; a finalized problem of the same solver takes poses
  // and points with ReloadParameterValues.  Throws std::runtime_error without poses or
  // factors, on a wrong anchor and on every refusal of ba_sim3_create.
  bool SolveSim3Graph(Options options, Summary *summary = nullptr, const std::vector<int> *point_anchors = nullptr,
                      std::vector<double> *scales = nullptr);
  // (new) s and w of the last SolveSim3Graph at the solved similarities, one entry per factor in
  // the order of AddRelativeSim3 (ba_sim3_factor_weights), as GetRelativeWeights: s in the
  // caller's units, w = 1 for a factor without a kernel.  Either output may be null.  Throws
  // std::runtime_error before the first SolveSim3Graph.
  void GetRelativeSim3Weights(std::vector<double> *s, std::vector<double> *w) const;
  // (new) ComputePoseGraphCovariance at width 7, on the graph that SolveSim3Graph solves at the
  // solver's current values, each pose the similarity (R, t, s = 1) (ba_sim3_covariance): tangent
  // [v; omega; sigma], the caller's units (sigma_pixel scaler)^2 D Sigma D with D = diag(100 I3,
  // I4), for the sigma_pixel the factors were added with (two values throw).  Returns false if
  // the factorisation dropped a pivot.
  bool ComputeSim3GraphCovariance(const std::vector<_BA_Pose *> &poses,
                                  const std::vector<std::pair<_BA_Pose *, _BA_Pose *>> &pairs,
                                  std::vector<Eigen::Matrix<double, 7, 7>> *cov_poses,
                                  std::vector<Eigen::Matrix<double, 7, 7>> *cov_cross,
                                  std::vector<Eigen::Matrix<double, 7, 7>> *cov_rel);
  // (new) GateLoopClosures at width 7 (ba_sim3_gate): (*d2)[c] in the caller's units, to be
  // compared with a chi-square quantile of 7 degrees of freedom (24.32 at 0.999).  A candidate
  // is a factor of AddRelativeSim3; its robust kernel, if any, is not read.
  bool GateSim3LoopClosures(const std::vector<RelativeSim3> &candidates, double sigma_pixel, std::vector<double> *d2);

  // (new) Solve the registered problems of several solver objects in ONE GPU launch
  // (ba_batch_solve of include/ba_hip.h: one persistent workgroup per problem runs the
  // whole LM loop; per problem at most 16 optimisable poses, 64 poses, 8 cameras).
  // Every solver's poses and points are written back as Solve writes them and
  // summaries (null, or resized to one Summary per solver) are filled.  A problem
  // beyond a limit or with non-finite values is left untouched and its Summary reports
  // convergence_status_ = false.  Returns true when every problem was solved.  The
  // solvers need not be finalized and are not finalized by this call; the first
  // solver's device is used.  Sharded solvers are refused (std::runtime_error).
  // in_priors (null: none): one PosePrior per solver, taken in as one more factor of its
  // problem (ba_batch_set_prior of include/ba_hip.h), H and b in the units MarginalizeBatch
  // returns for sigma_pixel.  in_relatives (null: none): one list of RelativePose factors per
  // solver (ba_batch_set_relative of include/ba_hip.h).  obs_masks (null: none): one flag
  // vector per solver (an empty one: none for that solver), one flag per observation the
  // solver registered, in registration order; an observation whose flag is 0 takes no part
  // (ba_batch_set_obs_mask of include/ba_hip.h).  cull (null: none): the two-stage local BA
  // in one go (ba_batch_solve_culled): the batch is solved with cull->first, every observation
  // whose squared error exceeds cull->chi2 * sigma_pixel^2 pixels^2 (or, with cull_behind,
  // that lies behind its camera) is switched off, and the batch is solved again with
  // `options`; cull_reports (null: not wanted) then gets one CullReport per solver, whose
  // `inliers` can be handed on as obs_masks of ComputeCovarianceBatch and MarginalizeBatch.
  // The Summary rows are those of both stages.
  struct PosePrior;
  struct RelativePose;
  struct CullOptions {
    Options first;
    double chi2 = 5.991;  // 95 % of a chi-square of two degrees of freedom
    bool cull_behind = true;
  };
  struct CullReport {
    std::vector<uint8_t> inliers;  // one per registered observation: 1 = still on
    int n_culled{0}, starved{0}, n_iter_first{0};
  };
  static bool SolveBatch(const std::vector<FullBundleAdjustmentSolver *> &solvers, Options options,
                         std::vector<Summary> *summaries = nullptr,
                         const std::vector<PosePrior> *in_priors = nullptr, double sigma_pixel = 1.0,
                         const std::vector<std::vector<RelativePose>> *in_relatives = nullptr,
                         const std::vector<std::vector<uint8_t>> *obs_masks = nullptr,
                         const CullOptions *cull = nullptr, std::vector<CullReport> *cull_reports = nullptr);

  // (new; the reference has no counterpart) Structure-only solve: EVERY registered pose is
  // treated as fixed and every non-fixed registered point is solved on its own against its
  // observations, all of them in one GPU launch (ba_point_only of include/ba_hip.h: its own
  // lambda, decisions and stop per point; options as in Solve).  The solver's current values
  // are used (after Solve: the solution).  triangulate: registered, non-fixed points whose
  // value is first replaced by a linear triangulation (it may be anything, NaN included); an
  // unknown or fixed pointer throws std::runtime_error.  A point with status 0 is written
  // back through the caller's pointer and becomes the solver's value (a finalized solver
  // continues from it); any other point is left as it was.  results (null: not wanted) gets
  // one entry per non-fixed point in registration order; costs are in the solver's scaled
  // units, as the rows of a Summary.  Poses are never touched.  The solver need not be
  // finalized and is not finalized by this call; sharded solvers are refused.  Returns true
  // when every point has status 0.
  struct PointOnlyResult {
    _BA_Point *point{nullptr};
    int n_iter{0}, converged{0}, status{0}, n_behind{0}, dropped_pivots{0};  // ba_point_result
    double cost0{0.0}, cost{0.0};
  };
  bool SolvePointsOnly(Options options, std::vector<PointOnlyResult> *results = nullptr,
                       const std::vector<_BA_Point *> &triangulate = std::vector<_BA_Point *>());

  // (new) Read the CURRENT values behind every registered pose / point pointer again
  // and hand them to the finalized problem (ba_update_values): re-optimising the same
  // graph with new values costs no second FinalizeParameters.  The reference keeps its
  // own copies from AddPose / AddPoint across Solve calls (.cpp:44-70, :87-117) and
  // has no such call; without it this class, like the reference, continues from its
  // internal state.
  void ReloadParameterValues();

  // (new; the reference has no counterpart) Covariance blocks of the CURRENT solver
  // state — after Solve: of the solution — for the given registered, optimisable poses
  // and points (any order, repeats allowed; either list may be empty), through
  // ba_covariance of include/ba_hip.h.  The blocks are those of sigma_pixel^2 (J^T W J)^-1
  // in the caller's units, W the Huber weights of a default Options (threshold 1.0): a pose
  // block is the covariance of the tangent xi = [v; omega] of the WORLD-TO-BODY pose
  // T_jw = inverse(*pose), left-multiplicative, T_jw <- exp(xi) T_jw (v in the caller's
  // length unit, omega in radians); a point block that of the world point.  With
  // D = diag(100 I3, I3) and the raw blocks Sigma_s of the scaled problem:
  // Cov_pose = sigma^2 1e-4 D Sigma_s D, Cov_point = sigma^2 Sigma_s.  Stereo: the solver's
  // own normal matrix is inverted (last-writer rule of the cross block, see ba_hip.h).
  // An unknown or fixed pointer throws std::runtime_error, as MakePoseFixed does.
  // Finalizes the parameters if that has not happened.  Returns true when the
  // factorisation met no non-positive pivot (false: S is singular, e.g. no fixed pose).
  bool ComputeCovariance(const std::vector<_BA_Pose *> &poses, const std::vector<_BA_Point *> &points,
                         double sigma_pixel, std::vector<Eigen::Matrix<double, 6, 6>> *cov_poses,
                         std::vector<Eigen::Matrix<double, 3, 3>> *cov_points);
  // (new) The covariance blocks of several solver objects in ONE launch
  // (ba_batch_covariance of include/ba_hip.h; the limits of SolveBatch per problem): for
  // solver b, cov_poses[b] holds one block per registered pose and cov_points[b] (null:
  // skipped) one per registered point, in registration order, at the solvers' CURRENT
  // values; blocks of fixed members are zero.  Units and conventions are those of
  // ComputeCovariance.  The solvers need not be finalized; the first solver's device is
  // used; sharded solvers are refused (std::runtime_error).  Returns true when every
  // problem has status 0 and its factorisation met no non-positive pivot.
  static bool ComputeCovarianceBatch(const std::vector<FullBundleAdjustmentSolver *> &solvers, double sigma_pixel,
                                     std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> *cov_poses,
                                     std::vector<std::vector<Eigen::Matrix<double, 3, 3>>> *cov_points,
                                     const std::vector<PosePrior> *in_priors = nullptr,
                                     const std::vector<std::vector<RelativePose>> *in_relatives = nullptr,
                                     const std::vector<std::vector<uint8_t>> *obs_masks = nullptr);
  // (new) The marginalisation prior one solver's window leaves on its kept poses: the
  // Gaussian 1/2 d^T H d - b^T d, d the stacked tangents xi = [v; omega] of the kept poses'
  // WORLD-TO-BODY transforms (the convention of ComputeCovariance), so that H d = b is their
  // Gauss-Newton step.  H is row-major dim x dim, dim = 6 * kept_poses.size(), symmetric to
  // the bit and in general singular (the gauge, poses that share no landmark with a marked one).
  struct MarginalPrior {
    int dim{0};
    std::vector<double> H, b;
    std::vector<_BA_Pose *> kept_poses;           // optimisable, unmarked; registration order
    std::vector<_BA_Point *> marginalized_points;  // the landmarks that leave with the marked poses
    int status{0}, dropped_pivots{0};              // ba_batch_marg_result of include/ba_hip.h
    // with in_relatives: one byte per factor of this solver, 1 where it joined and left with
    // the marked poses, 0 where the caller carries it into the next window
    std::vector<uint8_t> relatives_left;
    double operator()(int r, int c) const { return H[static_cast<size_t>(r) * dim + c]; }
  };
  // (new) The marginalisation priors of several solver objects in ONE launch
  // (ba_batch_marginalize of include/ba_hip.h; the limits of SolveBatch per problem), at the
  // solvers' CURRENT values: marg_poses[b] are the registered poses of solver b that leave
  // its window (fixed ones allowed: they own no columns but select their landmarks), every
  // optimisable landmark one of them observes leaves with them, and priors[b] is what the
  // observations of those landmarks leave on the other optimisable poses.  Units: the
  // caller's, for an isotropic pixel noise of sigma_pixel and the Huber weights of a default
  // Options; with D = diag(100 I3, I3) per pose and the raw H_s, b_s of the scaled problem,
  // H = D^-1 H_s D^-1 / (1e-4 sigma^2), b = D^-1 b_s / (1e-4 sigma^2): the inverse of the
  // conversion of ComputeCovariance.  An unknown pointer throws std::runtime_error; sharded
  // solvers are refused.  Returns true when every problem has status 0 and the elimination
  // of its marked poses met no non-positive pivot.
  static bool MarginalizeBatch(const std::vector<FullBundleAdjustmentSolver *> &solvers,
                               const std::vector<std::vector<_BA_Pose *>> &marg_poses, double sigma_pixel,
                               std::vector<MarginalPrior> *priors,
                               const std::vector<PosePrior> *in_priors = nullptr,
                               const std::vector<std::vector<RelativePose>> *in_relatives = nullptr,
                               const std::vector<std::vector<uint8_t>> *obs_masks = nullptr);
  // (new) A prior taken back IN by SolveBatch, ComputeCovarianceBatch and MarginalizeBatch
  // (in_priors, one per solver; an empty `poses` means none for that solver): the Gaussian
  // 1/2 d^T H d - b^T d + c / 2 on the registered, optimisable `poses`, in any order (the
  // blocks of H and b follow that order), d_j = log(T_jw inverse(T_jw at lin_poses[j])).
  // H (row-major, dim = 6 * poses.size()) and b in the units MarginalizeBatch returns for the
  // same sigma_pixel, c in the same units of energy (0, or b^T H^+ b); lin_poses are the
  // values at which H and b were formed, in the convention of AddPose and converted as
  // AddPose converts.  The derivative of d with respect to the update is taken as the
  // identity (first order, exact at d = 0): the caller keeps d small.  With a prior given,
  // MarginalizeBatch chains: the old prior joins the factors of the new one.
  struct PosePrior {
    std::vector<_BA_Pose *> poses;
    std::vector<double> H, b;
    std::vector<_BA_Pose> lin_poses;
    double c{0.0};
    PosePrior() = default;
    // what MarginalizeBatch returned, linearised at the CURRENT values of its kept poses
    explicit PosePrior(const MarginalPrior &m, double c_ = 0.0) : poses(m.kept_poses), H(m.H), b(m.b), c(c_) {
      for (const _BA_Pose *p : poses) lin_poses.push_back(*p);
    }
  };
  // (new) A relative-pose factor between two registered poses of one solver, taken in by
  // SolveBatch, ComputeCovarianceBatch and MarginalizeBatch (in_relatives, one list per solver):
  // odometry between keyframes, a loop closure, the pose part of an inertial delta.
  // measurement is the measured inverse(*pose_j) * (*pose_k) in the convention and units of
  // AddPose, that is T_jw T_kw^-1 of the world-to-body transforms after AddPose's conversion;
  // information is the row-major 6x6 information matrix of the tangent [v; omega] of those
  // transforms in the units MarginalizeBatch returns for the same sigma_pixel (only its lower
  // triangle is read).  Residual log(T_jw T_kw^-1 measurement^-1), Jacobians of first order
  // (identity and -Ad(T_jw T_kw^-1); exact at a zero residual), no robust weight.  The two
  // poses are distinct and not both fixed; a fixed pose receives nothing.  MarginalizeBatch
  // takes a factor in exactly when one of its poses is marked (MarginalPrior::relatives_left).
  struct RelativePose {
    _BA_Pose *pose_j{nullptr};
    _BA_Pose *pose_k{nullptr};
    _BA_Pose measurement;
    double information[36] = {0.0};
    // A robust kernel for SolvePoseGraph (include/ba_hip.h, ba_pgraph_set_robust): 0 none,
    // 1 Huber, 2 Cauchy, 3 Geman-McClure; robust_scale is the Mahalanobis distance c > 0 against
    // `information` in the caller's units.  Robust factors are pose-graph only: AddRelativePose
    // takes one (and throws on a kind outside 0..3 or a scale that is not finite or <= 0);
    // FinalizeParameters (Solve, ComputeCovariance) and the batch entry points throw
    // std::runtime_error on a factor that carries one.
    int robust_kind{0};
    double robust_scale{0.0};
  };
  // (new) A relative-pose factor of THIS solver's problem: an odometry or loop-closure edge
  // between two registered poses that Solve and ComputeCovariance then include
  // (ba_set_relative: any number of poses and factors, one GPU).  Units and conventions are
  // those of a factor of SolveBatch's in_relatives, converted for sigma_pixel in the same way.
  // Call before FinalizeParameters; afterwards it warns and is ignored, as AddPose.
  // ReloadParameterValues keeps the factors, Reset drops them.  Throws std::runtime_error on
  // a pose that was never registered; what the library refuses (the same pose twice, both
  // fixed, a non-finite value, a sharded solver) throws at FinalizeParameters.
  void AddRelativePose(const RelativePose &factor, double sigma_pixel = 1.0);
  // (new) Covariance blocks of the pose graph that SolvePoseGraph solves, at the solver's
  // current values; nothing is solved and FinalizeParameters is not needed
  // (ba_pgraph_covariance of include/ba_hip.h, the definition is there).  cov_poses[s]: the
  // marginal covariance of poses[s] (optimisable); for pairs[p] = {pose_j, pose_k}: cov_cross[p]
  // = Sigma_jk (may be null) and cov_rel[p], the covariance of the relative pose T_jw T_kw^-1,
  // first order, at lambda = 0.  Tangent and units as ComputeCovariance, for the sigma_pixel the
  // factors were added with: factors with different sigma_pixel throw std::runtime_error naming
  // the two values.  Returns false if the factorisation dropped a pivot (no fixed pose).
  bool ComputePoseGraphCovariance(const std::vector<_BA_Pose *> &poses,
                                  const std::vector<std::pair<_BA_Pose *, _BA_Pose *>> &pairs,
                                  std::vector<Eigen::Matrix<double, 6, 6>> *cov_poses,
                                  std::vector<Eigen::Matrix<double, 6, 6>> *cov_cross,
                                  std::vector<Eigen::Matrix<double, 6, 6>> *cov_rel);
  // (new) The chi-square gate for loop-closure candidates BEFORE they are added
  // (ba_pgraph_gate): (*d2)[c] = r^T (Sigma_E + information^-1)^-1 r of candidate c in the
  // caller's units, to be compared with a chi-square quantile of 6 degrees of freedom (22.46
  // at 0.999).  A candidate is a factor of AddRelativePose (no robust kernel), sigma_pixel the
  // one of the factors (std::runtime_error naming the two values otherwise).
  bool GateLoopClosures(const std::vector<RelativePose> &candidates, double sigma_pixel, std::vector<double> *d2);
  // the C-ABI handle behind the finalized problem (nullptr before FinalizeParameters):
  // for the readers of include/ba_hip.h; indices there are registration order
  ba_handle *GetHandle() const { return handle_; }

  std::string GetSolverStatistics() const;

  // GPU selection / console chatter (not in the reference)
  void SetDevice(int device_id) { device_id_ = device_id; }
  void SetVerbose(bool on) { verbose_ = on; }
  // Plain Gauss-Newton instead of Levenberg-Marquardt.  FullBundleAdjustmentSolver
  // itself never sets it (its Solve ignores options.solver_type, reference
  // :630-1044); FullBundleAdjustmentSolverRefactor does.
  void SetGaussNewton(bool on) { gauss_newton_ = on; }
  // Multi-GPU (new): this process owns landmark shard `rank` of
  // `world` (call before FinalizeParameters, with the SAME full problem
  // registered on every rank) and provides the sum-all-reduce the library calls
  // twice per LM iteration (ba_allreduce_fn of include/ba_hip.h; e.g.
  // multi_gpu::RcclAllReduce::Hook of utility/rccl_allreduce.h) and once more at
  // the end of Solve for the landmarks (ba_gather_points).  After Solve every rank
  // has written back all poses and ALL points (reference :1011-1022); OwnsPoint
  // tells which landmarks this rank linearised (all of them without a hook).
  void SetShard(int rank, int world) {
    shard_rank_ = rank;
    shard_world_ = world;
  }
  void SetAllReduce(int (*fn)(void *, int, void *, int64_t, void *), void *user);
  bool OwnsPoint(const _BA_Point *point) const;

 private:
  // SolveByGradientDescent of the refactored class runs through Run (same handle,
  // write-back and Summary as Solve)
  friend class FullBundleAdjustmentSolverRefactor;
  bool Run(Options options, Summary *summary, bool gradient_descent);
  // the solved values (scaled units, 12 doubles per pose, 3 per point) into the kept
  // copies and through the caller's pointers (:1011-1022); fixed members and points with
  // valid[q] == 0 are skipped.  Shared by Run and SolveBatch.
  void WriteBack(const double *T_jw12, const double *X3, const uint8_t *valid);
  // the concatenated arrays of ba_batch_create for a list of solvers (registered values,
  // not finalized state); shared by SolveBatch, ComputeCovarianceBatch and MarginalizeBatch
  struct BatchArrays {
    std::vector<int32_t> cam_off, pose_off, pt_off, oc, op, oq;
    std::vector<int64_t> obs_off;
    std::vector<double> intr, T_cj, T, X, uv;
    std::vector<uint8_t> pose_fixed, point_fixed;
  };
  static void PackBatch(const std::vector<FullBundleAdjustmentSolver *> &solvers, const char *who,
                        bool check_connectivity, BatchArrays *out);
  // ba_create + ba_batch_create on `device`; returns ba_batch_create's code (the caller
  // destroys both objects)
  static int CreateBatch(const BatchArrays &a, int device, ba_handle **h, ba_batch **batch);
  // obs_masks (may be null: returns false) into one flag per observation of the batch (an
  // empty vector of a solver: all on).  Throws std::runtime_error on a wrong size.
  static bool PackMasks(const BatchArrays &a, const char *who, const std::vector<std::vector<uint8_t>> *obs_masks,
                        std::vector<uint8_t> *flat);
  // in_priors (may be null: out->set stays false) into the arrays of ba_batch_set_prior:
  // scaled units, registration order.  Throws std::runtime_error on a malformed prior.
  struct PriorArrays {
    bool set{false};
    std::vector<int32_t> off, pose;
    std::vector<double> T_lin, H, b, c;
  };
  static void PackPriors(const std::vector<FullBundleAdjustmentSolver *> &solvers, const char *who,
                         const std::vector<PosePrior> *in_priors, double sigma_pixel, PriorArrays *out);
  static int SetPriors(ba_batch *batch, const PriorArrays &p);
  // in_relatives (may be null: out->set stays false) into the arrays of ba_batch_set_relative:
  // scaled units, registration indices.  Throws std::runtime_error on an unknown pointer.
  struct RelativeArrays {
    bool set{false};
    std::vector<int32_t> off, j, k;
    std::vector<double> Z, Omega;
    // AddRelativePose only: the robust kernels (scale in scaled units) and, per factor,
    // sigma_pixel * scaler, the unit of its Mahalanobis distance
    std::vector<int32_t> kind;
    std::vector<double> scale, unit;
  };
  static void PackRelatives(const std::vector<FullBundleAdjustmentSolver *> &solvers, const char *who,
                            const std::vector<std::vector<RelativePose>> *in_relatives, double sigma_pixel,
                            RelativeArrays *out);
  static int SetRelatives(ba_batch *batch, const RelativeArrays &r);
  // The factors of one graph, of AddRelativePose (Z 12, Omega 36 per factor) or of
  // AddRelativeSim3 (13, 49), in scaled units and input order (set and off unused), and s and w
  // of the graph's last solve.
  struct GraphFactors : RelativeArrays {
    std::vector<double> report_s, report_w;
  };
  GraphFactors relatives_, sim3_;
  // one Sim(3) factor or candidate into scaled units: Z (13) and Omega (49) appended
  void PackSim3(const RelativeSim3 &f, double sigma_pixel, std::vector<double> *Z, std::vector<double> *Omega) const;
  // The graph methods once, at the width of a kind (the traits Se3Abi: SolvePoseGraph and its
  // companions; Sim3Abi: SolveSim3Graph and its): in the .cpp, beside the traits
  template <class Abi>
  struct Graph;
  // the options' thresholds and iteration limit into a Summary (nullptr: nothing) and, after
  // the solve, its rows (Row: ba_iter_info of include/ba_hip.h), status and total time
  static void BeginSummary(Summary *summary, const Options &options);
  template <class Row>
  static void FinishSummary(Summary *summary, const std::vector<Row> &rows, int n_iter, int converged,
                            timer::StopWatch &stopwatch);
  // stderr warnings about weakly connected poses / points (reference
  // core/full_bundle_adjustment_solver.cpp:310-341), called by Solve
  void CheckPoseAndPointConnectivity();

  struct Observation {
    int camera_index;
    int pose_index;
    int point_index;
    double u, v;
  };
  _BA_Numeric scaler_{0.01};
  _BA_Numeric inverse_scaler_{100.0};
  bool is_parameter_finalized_{false};
  bool verbose_{true};
  bool gauss_newton_{false};
  int device_id_{0};
  ba_handle *handle_{nullptr};
  int shard_rank_{0}, shard_world_{1};
  int (*allreduce_fn_)(void *, int, void *, int64_t, void *){nullptr};
  void *allreduce_user_{nullptr};
  std::vector<uint8_t> owned_points_;  // filled by Solve (all ones on a single GPU)

  std::vector<_BA_Index> camera_ids_;
  std::vector<_BA_Camera> cameras_;  // scaled copies
  std::unordered_map<_BA_Pose *, int> pose_index_;
  std::vector<_BA_Pose *> poses_;
  std::vector<_BA_Pose> T_jw_;  // inverted + scaled
  std::unordered_set<int> fixed_poses_;
  std::unordered_map<_BA_Point *, int> point_index_;
  std::vector<_BA_Point *> points_;
  std::vector<_BA_Point> X_;  // scaled
  std::unordered_set<int> fixed_points_;
  std::vector<Observation> observations_;

  _BA_Size_t num_fixed_poses_{0};
  _BA_Size_t num_fixed_points_{0};
};

}  // namespace analytic_solver
}  // namespace visual_navigation
#endif
