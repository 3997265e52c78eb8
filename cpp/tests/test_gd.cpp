// GPU test driver of FullBundleAdjustmentSolverRefactor::SolveByGradientDescent:
// reads one problem from a text file, registers it through the reference's refactored
// signatures (core/full_bundle_adjustment_solver_refactor.h:117-136), solves it by
// gradient descent and prints poses, points and Summary rows for
// tests/test_gpu_gradient_descent.py to compare with the Python mirror.  Also checks
// that fixed objects are left untouched.  Exit code 0 = pass.
//
// input:  n_cam n_pose n_pt n_obs / per camera fx fy cx cy T_cb (12) /
//         per pose fixed T_wb (12) / per point fixed X (3) /
//         per observation cam pose point u v /
//         max_iter thr_step thr_cost huber lambda0     (12 = R row-major then t)
#include <cstdio>
#include <fstream>
#include <vector>

#include "core/full_bundle_adjustment_solver_refactor.h"
#include "eigen3/Eigen/Dense"

using namespace visual_navigation::analytic_solver;

static Pose Read12(std::istream &in) {
  Pose T = Pose::Identity();
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) in >> T.linear()(r, c);
  for (int r = 0; r < 3; ++r) in >> T.translation()(r);
  return T;
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: test_gd problem.txt\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  int n_cam = 0, n_pose = 0, n_pt = 0, n_obs = 0;
  in >> n_cam >> n_pose >> n_pt >> n_obs;
  FullBundleAdjustmentSolverRefactor solver;
  solver.SetVerbose(false);
  for (int c = 0; c < n_cam; ++c) {
    OptimizerCamera cam;
    in >> cam.fx >> cam.fy >> cam.cx >> cam.cy;
    cam.camera_to_body_pose = Read12(in);
    solver.RegisterCamera(c, cam);
  }
  std::vector<Pose> poses(n_pose);
  std::vector<Point> points(n_pt);
  std::vector<int> pose_fixed(n_pose), pt_fixed(n_pt);
  for (int j = 0; j < n_pose; ++j) {
    in >> pose_fixed[j];
    poses[j] = Read12(in);
  }
  for (int i = 0; i < n_pt; ++i) in >> pt_fixed[i] >> points[i](0) >> points[i](1) >> points[i](2);
  for (int j = 0; j < n_pose; ++j) solver.RegisterWorldToBodyPose(&poses[j]);
  for (int i = 0; i < n_pt; ++i) solver.RegisterWorldPoint(&points[i]);
  for (int j = 0; j < n_pose; ++j)
    if (pose_fixed[j]) solver.MakePoseFixed(&poses[j]);
  for (int i = 0; i < n_pt; ++i)
    if (pt_fixed[i]) solver.MakePointFixed(&points[i]);
  for (int k = 0; k < n_obs; ++k) {
    int c, j, i;
    Pixel uv;
    in >> c >> j >> i >> uv(0) >> uv(1);
    solver.AddObservation(c, &poses[j], &points[i], uv);
  }
  Options options;
  in >> options.iteration_handle.max_num_iterations >> options.convergence_handle.threshold_step_size >>
      options.convergence_handle.threshold_cost_change >> options.outlier_handle.threshold_huber_loss >>
      options.trust_region_handle.initial_lambda;
  if (!in) {
    std::printf("bad input file\n");
    return 2;
  }
  const std::vector<Pose> poses0 = poses;
  const std::vector<Point> points0 = points;
  Summary summary;
  const bool ok = solver.SolveByGradientDescent(options, &summary);
  int fail = ok ? 0 : 1;
  // fixed objects: bit for bit untouched
  for (int j = 0; j < n_pose; ++j)
    for (int r = 0; r < 3 && pose_fixed[j]; ++r)
      for (int c = 0; c < 4; ++c)
        if (poses[j].matrix()(r, c) != poses0[j].matrix()(r, c)) ++fail;
  for (int i = 0; i < n_pt; ++i)
    for (int r = 0; r < 3 && pt_fixed[i]; ++r)
      if (points[i](r) != points0[i](r)) ++fail;
  std::printf("converged %d\n", summary.IsConverged() ? 1 : 0);
  for (const auto &r : summary.GetOptimizationInfoList())
    std::printf("row %.17e %.17e %.17e %.17e %.17e %.17e %d\n", r.cost, r.cost_change, r.average_reprojection_error,
                r.abs_step, r.abs_gradient, r.damping_term, static_cast<int>(r.iteration_status));
  for (int j = 0; j < n_pose; ++j) {
    std::printf("pose");
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) std::printf(" %.17e", poses[j].matrix()(r, c));
    std::printf("\n");
  }
  for (int i = 0; i < n_pt; ++i) std::printf("point %.17e %.17e %.17e\n", points[i](0), points[i](1), points[i](2));
  std::printf(fail ? "GD FACADE TEST FAILED (%d)\n" : "GD FACADE TEST PASSED\n", fail);
  return fail ? 1 : 0;
}
