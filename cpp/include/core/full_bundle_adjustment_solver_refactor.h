// FullBundleAdjustmentSolverRefactor — host facade with the refactored names of
// the reference (core/full_bundle_adjustment_solver_refactor.h:36-136): the same
// device path as FullBundleAdjustmentSolver behind RegisterCamera /
// RegisterWorldToBodyPose / RegisterWorldPoint, plus the solver_type switch of
// its Solve (reference ..._refactor.cpp:944-982) and its first-order
// SolveByGradientDescent (:1075-1367, ba_solve_gd).  Reference test/
// test_ba_refactor.cpp compiles against this header unchanged.
#ifndef BA_FACADE_FULL_BUNDLE_ADJUSTMENT_SOLVER_REFACTOR_H_
#define BA_FACADE_FULL_BUNDLE_ADJUSTMENT_SOLVER_REFACTOR_H_

#include <string>
#include <vector>

#include "core/full_bundle_adjustment_solver.h"
#include "core/solver_option_and_summary.h"
#include "eigen3/Eigen/Dense"
#include "utility/timer.h"

namespace visual_navigation {
namespace analytic_solver {

// scalar / vector aliases of the refactored API (same names, reference :36-51)
typedef double SolverNumeric;
typedef int Index;
typedef Eigen::Matrix<SolverNumeric, 2, 1> Pixel;          // image point [pixel]
typedef Eigen::Matrix<SolverNumeric, 3, 1> Point;          // world point [m]
typedef Eigen::Matrix<SolverNumeric, 3, 3> Rotation3D;
typedef Eigen::Matrix<SolverNumeric, 3, 1> Translation3D;
typedef Eigen::Transform<SolverNumeric, 3, 1> Pose;        // rigid (Isometry) transform
typedef std::vector<SolverNumeric> ErrorList;
typedef std::vector<Index> IndexList;
typedef std::vector<Pixel> PixelList;
typedef std::vector<Point> PointList;

// Pinhole camera of the rig.  camera_to_body_pose is applied as
// X_camera = camera_to_body_pose * X_body (reference ..._refactor.cpp:758).
struct OptimizerCamera {
  OptimizerCamera() = default;
  OptimizerCamera(const OptimizerCamera &other) = default;
  OptimizerCamera &operator=(const OptimizerCamera &other) = default;
  SolverNumeric fx = 0.0, fy = 0.0;  // focal lengths [pixel]
  SolverNumeric cx = 0.0, cy = 0.0;  // principal point [pixel]
  Pose camera_to_body_pose;
};

// One pixel measurement of a point from a pose through a camera.
struct PointObservation {
  int related_camera_id = -1;
  Pose *related_pose = nullptr;
  Point *related_point = nullptr;
  Pixel pixel{-1.0, -1.0};
};

class FullBundleAdjustmentSolverRefactor {
 public:
  FullBundleAdjustmentSolverRefactor();

  void Reset();

  void RegisterCamera(const Index camera_id, const OptimizerCamera &camera);
  void RegisterWorldToBodyPose(Pose *original_pose);
  void RegisterWorldPoint(Point *original_point);

  void MakePoseFixed(Pose *original_pose);
  void MakePointFixed(Point *original_point);

  // solver_type LEVENBERG_MARQUARDT or GAUSS_NEWTON (the default of Options);
  // anything else throws std::runtime_error
  bool Solve(Options options, Summary *summary = nullptr);
  // reference ..._refactor.cpp:1075-1367 (ba_solve_gd): first-order steps, each pose /
  // point block clipped to norm 1e-3 in the solver's scaled units, every step taken;
  // solver_type and the lambda ratios are ignored, damping_term = initial_lambda
  bool SolveByGradientDescent(Options options, Summary *summary = nullptr);
  // (new) pose-graph optimisation over the factors of AddRelativePose alone, see
  // FullBundleAdjustmentSolver::SolvePoseGraph; solver_type selects Levenberg-Marquardt or
  // Gauss-Newton as in Solve, for this call only
  bool SolvePoseGraph(Options options, Summary *summary = nullptr);
  // (new) the Sim(3) pose graph, see FullBundleAdjustmentSolver::AddRelativeSim3 and
  // SolveSim3Graph; solver_type selects Levenberg-Marquardt or Gauss-Newton as in Solve, for
  // this call only
  using RelativeSim3 = FullBundleAdjustmentSolver::RelativeSim3;
  void AddRelativeSim3(const RelativeSim3 &factor, double sigma_pixel = 1.0) {
    impl_.AddRelativeSim3(factor, sigma_pixel);
  }
  bool SolveSim3Graph(Options options, Summary *summary = nullptr, const std::vector<int> *point_anchors = nullptr,
                      std::vector<double> *scales = nullptr);
  // (new) see FullBundleAdjustmentSolver::GetRelativeSim3Weights, ComputeSim3GraphCovariance and
  // GateSim3LoopClosures
  void GetRelativeSim3Weights(std::vector<double> *s, std::vector<double> *w) const {
    impl_.GetRelativeSim3Weights(s, w);
  }
  bool ComputeSim3GraphCovariance(const std::vector<Pose *> &poses, const std::vector<std::pair<Pose *, Pose *>> &pairs,
                                  std::vector<Eigen::Matrix<double, 7, 7>> *cov_poses,
                                  std::vector<Eigen::Matrix<double, 7, 7>> *cov_cross,
                                  std::vector<Eigen::Matrix<double, 7, 7>> *cov_rel) {
    return impl_.ComputeSim3GraphCovariance(poses, pairs, cov_poses, cov_cross, cov_rel);
  }
  bool GateSim3LoopClosures(const std::vector<RelativeSim3> &candidates, double sigma_pixel, std::vector<double> *d2) {
    return impl_.GateSim3LoopClosures(candidates, sigma_pixel, d2);
  }
  // (new) see FullBundleAdjustmentSolver::GetRelativeWeights
  void GetRelativeWeights(std::vector<double> *s, std::vector<double> *w) const { impl_.GetRelativeWeights(s, w); }
  // (new) see FullBundleAdjustmentSolver::ComputePoseGraphCovariance and GateLoopClosures
  bool ComputePoseGraphCovariance(const std::vector<Pose *> &poses, const std::vector<std::pair<Pose *, Pose *>> &pairs,
                                  std::vector<Eigen::Matrix<double, 6, 6>> *cov_poses,
                                  std::vector<Eigen::Matrix<double, 6, 6>> *cov_cross,
                                  std::vector<Eigen::Matrix<double, 6, 6>> *cov_rel) {
    return impl_.ComputePoseGraphCovariance(poses, pairs, cov_poses, cov_cross, cov_rel);
  }
  bool GateLoopClosures(const std::vector<FullBundleAdjustmentSolver::RelativePose> &candidates, double sigma_pixel,
                        std::vector<double> *d2) {
    return impl_.GateLoopClosures(candidates, sigma_pixel, d2);
  }

  // (new) covariance blocks of the current state, see FullBundleAdjustmentSolver::ComputeCovariance:
  // same units, same tangent convention (world-to-body T_jw = inverse(*pose), T_jw <- exp(xi) T_jw)
  bool ComputeCovariance(const std::vector<Pose *> &poses, const std::vector<Point *> &points, double sigma_pixel,
                         std::vector<Eigen::Matrix<double, 6, 6>> *cov_poses,
                         std::vector<Eigen::Matrix<double, 3, 3>> *cov_points) {
    return impl_.ComputeCovariance(poses, points, sigma_pixel, cov_poses, cov_points);
  }
  // (new) the blocks of several solvers in one launch, see
  // FullBundleAdjustmentSolver::ComputeCovarianceBatch
  static bool ComputeCovarianceBatch(const std::vector<FullBundleAdjustmentSolverRefactor *> &solvers,
                                     double sigma_pixel,
                                     std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> *cov_poses,
                                     std::vector<std::vector<Eigen::Matrix<double, 3, 3>>> *cov_points) {
    std::vector<FullBundleAdjustmentSolver *> impls;
    for (FullBundleAdjustmentSolverRefactor *s : solvers) impls.push_back(s ? &s->impl_ : nullptr);
    return FullBundleAdjustmentSolver::ComputeCovarianceBatch(impls, sigma_pixel, cov_poses, cov_points);
  }
  // the same with one pose prior per solver taken in, see FullBundleAdjustmentSolver::PosePrior
  using PosePrior = FullBundleAdjustmentSolver::PosePrior;
  static bool ComputeCovarianceBatch(const std::vector<FullBundleAdjustmentSolverRefactor *> &solvers,
                                     double sigma_pixel,
                                     std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> *cov_poses,
                                     std::vector<std::vector<Eigen::Matrix<double, 3, 3>>> *cov_points,
                                     const std::vector<PosePrior> *in_priors) {
    std::vector<FullBundleAdjustmentSolver *> impls;
    for (FullBundleAdjustmentSolverRefactor *s : solvers) impls.push_back(s ? &s->impl_ : nullptr);
    return FullBundleAdjustmentSolver::ComputeCovarianceBatch(impls, sigma_pixel, cov_poses, cov_points, in_priors);
  }
  // (new) the marginalisation priors of several solvers in one launch, see
  // FullBundleAdjustmentSolver::MarginalizeBatch
  using MarginalPrior = FullBundleAdjustmentSolver::MarginalPrior;
  static bool MarginalizeBatch(const std::vector<FullBundleAdjustmentSolverRefactor *> &solvers,
                               const std::vector<std::vector<Pose *>> &marg_poses, double sigma_pixel,
                               std::vector<MarginalPrior> *priors) {
    std::vector<FullBundleAdjustmentSolver *> impls;
    for (FullBundleAdjustmentSolverRefactor *s : solvers) impls.push_back(s ? &s->impl_ : nullptr);
    return FullBundleAdjustmentSolver::MarginalizeBatch(impls, marg_poses, sigma_pixel, priors);
  }
  static bool MarginalizeBatch(const std::vector<FullBundleAdjustmentSolverRefactor *> &solvers,
                               const std::vector<std::vector<Pose *>> &marg_poses, double sigma_pixel,
                               std::vector<MarginalPrior> *priors, const std::vector<PosePrior> *in_priors) {
    std::vector<FullBundleAdjustmentSolver *> impls;
    for (FullBundleAdjustmentSolverRefactor *s : solvers) impls.push_back(s ? &s->impl_ : nullptr);
    return FullBundleAdjustmentSolver::MarginalizeBatch(impls, marg_poses, sigma_pixel, priors, in_priors);
  }
  // (new) relative-pose factors between registered poses, see
  // FullBundleAdjustmentSolver::RelativePose; one list per solver.  SolveBatch: see
  // FullBundleAdjustmentSolver::SolveBatch; options.solver_type selects Levenberg-Marquardt
  // or Gauss-Newton as in Solve (anything else throws std::runtime_error), for this call only:
  // what an earlier Solve selected is put back afterwards.
  using RelativePose = FullBundleAdjustmentSolver::RelativePose;
  // (new) the two-stage local BA of SolveBatch, see FullBundleAdjustmentSolver::CullOptions
  using CullOptions = FullBundleAdjustmentSolver::CullOptions;
  using CullReport = FullBundleAdjustmentSolver::CullReport;
  // (new) a relative-pose factor of this solver's own problem, see
  // FullBundleAdjustmentSolver::AddRelativePose
  void AddRelativePose(const RelativePose &factor, double sigma_pixel = 1.0) {
    impl_.AddRelativePose(factor, sigma_pixel);
  }
  static bool SolveBatch(const std::vector<FullBundleAdjustmentSolverRefactor *> &solvers, Options options,
                         std::vector<Summary> *summaries = nullptr,
                         const std::vector<PosePrior> *in_priors = nullptr, double sigma_pixel = 1.0,
                         const std::vector<std::vector<RelativePose>> *in_relatives = nullptr,
                         const std::vector<std::vector<uint8_t>> *obs_masks = nullptr,
                         const CullOptions *cull = nullptr, std::vector<CullReport> *cull_reports = nullptr);
  // obs_masks (last, null: none): one flag per registered observation of every solver, see
  // FullBundleAdjustmentSolver::SolveBatch
  static bool ComputeCovarianceBatch(const std::vector<FullBundleAdjustmentSolverRefactor *> &solvers,
                                     double sigma_pixel,
                                     std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> *cov_poses,
                                     std::vector<std::vector<Eigen::Matrix<double, 3, 3>>> *cov_points,
                                     const std::vector<PosePrior> *in_priors,
                                     const std::vector<std::vector<RelativePose>> *in_relatives,
                                     const std::vector<std::vector<uint8_t>> *obs_masks = nullptr) {
    std::vector<FullBundleAdjustmentSolver *> impls;
    for (FullBundleAdjustmentSolverRefactor *s : solvers) impls.push_back(s ? &s->impl_ : nullptr);
    return FullBundleAdjustmentSolver::ComputeCovarianceBatch(impls, sigma_pixel, cov_poses, cov_points, in_priors,
                                                              in_relatives, obs_masks);
  }
  static bool MarginalizeBatch(const std::vector<FullBundleAdjustmentSolverRefactor *> &solvers,
                               const std::vector<std::vector<Pose *>> &marg_poses, double sigma_pixel,
                               std::vector<MarginalPrior> *priors, const std::vector<PosePrior> *in_priors,
                               const std::vector<std::vector<RelativePose>> *in_relatives,
                               const std::vector<std::vector<uint8_t>> *obs_masks = nullptr) {
    std::vector<FullBundleAdjustmentSolver *> impls;
    for (FullBundleAdjustmentSolverRefactor *s : solvers) impls.push_back(s ? &s->impl_ : nullptr);
    return FullBundleAdjustmentSolver::MarginalizeBatch(impls, marg_poses, sigma_pixel, priors, in_priors,
                                                        in_relatives, obs_masks);
  }
  // (new) structure-only solve, see FullBundleAdjustmentSolver::SolvePointsOnly;
  // options.solver_type selects Levenberg-Marquardt or Gauss-Newton as in Solve (anything
  // else throws std::runtime_error), for this call only
  using PointOnlyResult = FullBundleAdjustmentSolver::PointOnlyResult;
  bool SolvePointsOnly(Options options, std::vector<PointOnlyResult> *results = nullptr,
                       const std::vector<Point *> &triangulate = std::vector<Point *>());
  ba_handle *GetHandle() const { return impl_.GetHandle(); }

  std::string GetSolverStatistics() const;

  void AddObservation(const Index camera_id, Pose *related_pose, Point *related_point, const Pixel &pixel);

  void SetDevice(int device_id) { impl_.SetDevice(device_id); }
  void SetVerbose(bool on) { impl_.SetVerbose(on); }

 private:
  FullBundleAdjustmentSolver impl_;
};

}  // namespace analytic_solver
}  // namespace visual_navigation
#endif
