// GPU test driver of the planar 3-DoF pose-only facade: reads one problem from a
// text file, solves it through
// visual_navigation::analytic_solver::PoseOnlyBundleAdjustmentSolver::
// Solve_Monocular_Planar3Dof or ::Solve_Stereo_Planar3Dof with the reference's
// signatures (core/pose_only_bundle_adjustment_solver.h:28-48), and prints the
// results for tests/test_gpu_planar_pose_only.py to compare with the Python
// mirror.  Also checks the facade-only behaviour (size-mismatch exceptions,
// n = 0, debug poses).  Exit code 0 = pass.
//
// input:  n stereo / fx fy cx cy / T_bc (12) / T_lr (12) / T_wl (12) / T_wc (12) /
//         max_iter thr_step thr_cost huber outlier / n lines of X (3) uv (2) uvr (2)
//         (12 = R row-major then t)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "core/pose_only_bundle_adjustment_solver.h"
#include "eigen3/Eigen/Dense"
#include "eigen3/Eigen/Geometry"

using namespace visual_navigation::analytic_solver;

static int g_fail = 0;
#define EXPECT(cond, ...)                              \
  do {                                                 \
    if (!(cond)) {                                     \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                        \
      std::printf("\n");                               \
      ++g_fail;                                        \
    }                                                  \
  } while (0)

static Eigen::Isometry3f Read12(std::istream &in) {
  Eigen::Isometry3f T;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) in >> T.linear()(r, c);
  for (int r = 0; r < 3; ++r) in >> T.translation()(r);
  return T;
}

static void Print12(const char *tag, const Eigen::Isometry3f &T) {
  std::printf("%s", tag);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) std::printf(" %.9e", T.linear()(r, c));
  for (int r = 0; r < 3; ++r) std::printf(" %.9e", T.translation()(r));
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: test_planar <problem.txt>\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  int n = 0, stereo = 0;
  float fx, fy, cx, cy;
  in >> n >> stereo >> fx >> fy >> cx >> cy;
  const Eigen::Isometry3f T_bc = Read12(in), T_lr = Read12(in), T_wl = Read12(in);
  const Eigen::Isometry3f T_wc = Read12(in);
  Options options;
  in >> options.iteration_handle.max_num_iterations >> options.convergence_handle.threshold_step_size >>
      options.convergence_handle.threshold_cost_change >> options.outlier_handle.threshold_huber_loss >>
      options.outlier_handle.threshold_outlier_rejection;
  std::vector<Eigen::Vector3f> X(n);
  std::vector<Eigen::Vector2f> uvl(n), uvr(n);
  for (int k = 0; k < n; ++k) in >> X[k](0) >> X[k](1) >> X[k](2) >> uvl[k](0) >> uvl[k](1) >> uvr[k](0) >> uvr[k](1);
  if (!in) {
    std::printf("FAIL: could not read %s\n", argv[1]);
    return 2;
  }

  PoseOnlyBundleAdjustmentSolver solver;
  Summary summary;
  Eigen::Isometry3f pose = T_wc;
  std::vector<bool> ml, mr;
  bool ok;
  if (stereo)
    ok = solver.Solve_Stereo_Planar3Dof(X, uvl, uvr, fx, fy, cx, cy, fx, fy, cx, cy, T_bc, T_lr, T_wl, pose, ml, mr,
                                        options, &summary);
  else
    ok = solver.Solve_Monocular_Planar3Dof(X, uvl, fx, fy, cx, cy, T_bc, T_wl, pose, ml, options, &summary);
  const auto &rows = summary.GetOptimizationInfoList();
  const auto &dbg = solver.GetDebugPoses();
  std::printf("success %d\nconverged %d\nn_debug %zu\nn_rows %zu\n", ok ? 1 : 0,
              summary.IsConverged() ? 1 : 0, dbg.size(), rows.size());
  Print12("T12", pose);
  for (const auto &r : rows) std::printf("row %.9e %.9e %.9e\n", r.cost, r.cost_change, r.abs_step);
  std::printf("mask_l");
  for (int k = 0; k < n; ++k) std::printf("%d", ml[k] ? 1 : 0);
  std::printf("\nmask_r");
  for (size_t k = 0; k < mr.size(); ++k) std::printf("%d", mr[k] ? 1 : 0);
  std::printf("\n");
  EXPECT((int)ml.size() == n && (!stereo || (int)mr.size() == n), "masks resized to n");
  if (ok && !dbg.empty()) {
    float d = 0.0f;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) d = std::max(d, std::abs(dbg.back().linear()(r, c) - pose.linear()(r, c)));
      d = std::max(d, std::abs(dbg.back().translation()(r) - pose.translation()(r)));
    }
    EXPECT(d == 0.0f, "last debug pose != written pose (%g)", d);
  }

  // size mismatch throws with the reference's message (:426-432, :647-660)
  const std::vector<Eigen::Vector2f> short_uv(uvl.begin(), uvl.end() - 1);
  int thrown = 0;
  Eigen::Isometry3f p2 = T_wc;
  try {
    solver.Solve_Monocular_Planar3Dof(X, short_uv, fx, fy, cx, cy, T_bc, T_wl, p2, ml, options);
  } catch (const std::runtime_error &e) {
    thrown += std::string(e.what()).find("!= current_pixel_list.size()") != std::string::npos;
  }
  try {
    solver.Solve_Stereo_Planar3Dof(X, uvl, short_uv, fx, fy, cx, cy, fx, fy, cx, cy, T_bc, T_lr, T_wl, p2, ml, mr,
                                   options);
  } catch (const std::runtime_error &e) {
    thrown += std::string(e.what()).find("!= right_current_pixel_list.size()") != std::string::npos;
  }
  EXPECT(thrown == 2, "size mismatch must throw (%d of 2)", thrown);
  // n = 0: pose unchanged, true (as the 6-DoF facade)
  std::vector<bool> m0;
  EXPECT(solver.Solve_Monocular_Planar3Dof({}, {}, fx, fy, cx, cy, T_bc, T_wl, p2, m0, options) &&
             solver.GetDebugPoses().empty(),
         "n = 0");
  if (g_fail == 0) std::printf("PLANAR FACADE TEST PASSED\n");
  return g_fail == 0 ? 0 : 1;
}
