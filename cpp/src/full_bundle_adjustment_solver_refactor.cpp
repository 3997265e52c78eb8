// See the header.  Reference line numbers: core/full_bundle_adjustment_solver_refactor.cpp.
#include "core/full_bundle_adjustment_solver_refactor.h"

#include <stdexcept>

namespace visual_navigation {
namespace analytic_solver {

FullBundleAdjustmentSolverRefactor::FullBundleAdjustmentSolverRefactor() {}

void FullBundleAdjustmentSolverRefactor::Reset() { impl_.Reset(); }

void FullBundleAdjustmentSolverRefactor::RegisterCamera(const Index camera_id, const OptimizerCamera &camera) {  // :68-94
  _BA_Camera c;
  c.fx = camera.fx;
  c.fy = camera.fy;
  c.cx = camera.cx;
  c.cy = camera.cy;
  c.pose_this_to_cam0 = camera.camera_to_body_pose;  // same role: X_c = T * X_body (:758 vs full_...cpp:746)
  impl_.AddCamera(camera_id, c);
}

void FullBundleAdjustmentSolverRefactor::RegisterWorldToBodyPose(Pose *original_pose) {  // :96-111
  impl_.AddPose(original_pose);
}

void FullBundleAdjustmentSolverRefactor::RegisterWorldPoint(Point *original_point) {  // :113-126
  impl_.AddPoint(original_point);
}

void FullBundleAdjustmentSolverRefactor::MakePoseFixed(Pose *original_pose) { impl_.MakePoseFixed(original_pose); }
void FullBundleAdjustmentSolverRefactor::MakePointFixed(Point *original_point) { impl_.MakePointFixed(original_point); }

void FullBundleAdjustmentSolverRefactor::AddObservation(const Index camera_id, Pose *related_pose,
                                                        Point *related_point, const Pixel &pixel) {
  impl_.AddObservation(camera_id, related_pose, related_point, pixel);
}

bool FullBundleAdjustmentSolverRefactor::Solve(Options options, Summary *summary) {  // :640-1071
  if (options.solver_type == SolverType::LEVENBERG_MARQUARDT)
    impl_.SetGaussNewton(false);
  else if (options.solver_type == SolverType::GAUSS_NEWTON)
    impl_.SetGaussNewton(true);  // :976-982: every step accepted, lambda stays at initial_lambda
  else
    throw std::runtime_error(
        "FullBundleAdjustmentSolverRefactor::Solve: solver_type must be GAUSS_NEWTON or LEVENBERG_MARQUARDT");
  return impl_.Solve(options, summary);
}

bool FullBundleAdjustmentSolverRefactor::SolveBatch(const std::vector<FullBundleAdjustmentSolverRefactor *> &solvers,
                                                    Options options, std::vector<Summary> *summaries,
                                                    const std::vector<PosePrior> *in_priors, double sigma_pixel,
                                                    const std::vector<std::vector<RelativePose>> *in_relatives,
                                                    const std::vector<std::vector<uint8_t>> *obs_masks,
                                                    const CullOptions *cull, std::vector<CullReport> *cull_reports) {
  if (options.solver_type != SolverType::LEVENBERG_MARQUARDT && options.solver_type != SolverType::GAUSS_NEWTON)
    throw std::runtime_error(
        "FullBundleAdjustmentSolverRefactor::SolveBatch: solver_type must be GAUSS_NEWTON or LEVENBERG_MARQUARDT");
  // the mode holds for this call only: what Solve set before stays for the next Solve
  std::vector<FullBundleAdjustmentSolver *> impls;
  std::vector<bool> before;
  for (FullBundleAdjustmentSolverRefactor *s : solvers) {
    impls.push_back(s ? &s->impl_ : nullptr);
    before.push_back(s ? s->impl_.gauss_newton_ : false);
    if (s) s->impl_.SetGaussNewton(options.solver_type == SolverType::GAUSS_NEWTON);
  }
  const auto restore = [&] {
    for (size_t k = 0; k < impls.size(); ++k)
      if (impls[k]) impls[k]->SetGaussNewton(before[k]);
  };
  bool ok = false;
  try {
    ok = FullBundleAdjustmentSolver::SolveBatch(impls, options, summaries, in_priors, sigma_pixel, in_relatives,
                                                obs_masks, cull, cull_reports);
  } catch (...) {
    restore();
    throw;
  }
  restore();
  return ok;
}

bool FullBundleAdjustmentSolverRefactor::SolvePointsOnly(Options options, std::vector<PointOnlyResult> *results,
                                                         const std::vector<Point *> &triangulate) {
  if (options.solver_type != SolverType::LEVENBERG_MARQUARDT && options.solver_type != SolverType::GAUSS_NEWTON)
    throw std::runtime_error(
        "FullBundleAdjustmentSolverRefactor::SolvePointsOnly: solver_type must be GAUSS_NEWTON or LEVENBERG_MARQUARDT");
  const bool before = impl_.gauss_newton_;  // the mode holds for this call only
  impl_.SetGaussNewton(options.solver_type == SolverType::GAUSS_NEWTON);
  bool ok = false;
  try {
    ok = impl_.SolvePointsOnly(options, results, triangulate);
  } catch (...) {
    impl_.SetGaussNewton(before);
    throw;
  }
  impl_.SetGaussNewton(before);
  return ok;
}

bool FullBundleAdjustmentSolverRefactor::SolvePoseGraph(Options options, Summary *summary) {
  if (options.solver_type != SolverType::LEVENBERG_MARQUARDT && options.solver_type != SolverType::GAUSS_NEWTON)
    throw std::runtime_error(
        "FullBundleAdjustmentSolverRefactor::SolvePoseGraph: solver_type must be GAUSS_NEWTON or LEVENBERG_MARQUARDT");
  const bool before = impl_.gauss_newton_;  // the mode holds for this call only
  impl_.SetGaussNewton(options.solver_type == SolverType::GAUSS_NEWTON);
  bool ok = false;
  try {
    ok = impl_.SolvePoseGraph(options, summary);
  } catch (...) {
    impl_.SetGaussNewton(before);
    throw;
  }
  impl_.SetGaussNewton(before);
  return ok;
}

bool FullBundleAdjustmentSolverRefactor::SolveSim3Graph(Options options, Summary *summary,
                                                        const std::vector<int> *point_anchors,
                                                        std::vector<double> *scales) {
  if (options.solver_type != SolverType::LEVENBERG_MARQUARDT && options.solver_type != SolverType::GAUSS_NEWTON)
    throw std::runtime_error(
        "FullBundleAdjustmentSolverRefactor::SolveSim3Graph: solver_type must be GAUSS_NEWTON or LEVENBERG_MARQUARDT");
  const bool before = impl_.gauss_newton_;  // the mode holds for this call only
  impl_.SetGaussNewton(options.solver_type == SolverType::GAUSS_NEWTON);
  bool ok = false;
  try {
    ok = impl_.SolveSim3Graph(options, summary, point_anchors, scales);
  } catch (...) {
    impl_.SetGaussNewton(before);
    throw;
  }
  impl_.SetGaussNewton(before);
  return ok;
}

bool FullBundleAdjustmentSolverRefactor::SolveByGradientDescent(Options options, Summary *summary) {  // :1075-1367
  return impl_.Run(options, summary, true);
}

std::string FullBundleAdjustmentSolverRefactor::GetSolverStatistics() const { return impl_.GetSolverStatistics(); }

}  // namespace analytic_solver
}  // namespace visual_navigation
