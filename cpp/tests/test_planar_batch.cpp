// GPU test driver of the batched planar 3-DoF pose-only facade: reads B frames
// from a text file, solves them in one call of
// visual_navigation::analytic_solver::PoseOnlyBundleAdjustmentSolver::
// Solve_Monocular_Planar3Dof_Batch or ::Solve_Stereo_Planar3Dof_Batch, and
// prints every frame's results for tests/test_gpu_planar_batch.py to compare
// with the Python mirror.  Also checks the facade-only behaviour (size-mismatch
// exception before any device use, frames without points).  Exit code 0 = pass.
//
// input:  B stereo / max_iter thr_step thr_cost huber outlier / per frame:
//         n fx fy cx cy / T_bc (12) / T_lr (12) / T_wl (12) / T_wc_init (12) /
//         n lines of X (3) uv (2) uvr (2)
//         (12 = R row-major then t; the right camera uses the left intrinsics)
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
using Solver = PoseOnlyBundleAdjustmentSolver;

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

static void Print(int b, const Eigen::Isometry3f &T, bool ok, const Summary &s, const std::vector<bool> &ml,
                  const std::vector<bool> *mr) {
  const auto &rows = s.GetOptimizationInfoList();
  std::printf("frame %d success %d converged %d n_rows %zu\n", b, ok ? 1 : 0, s.IsConverged() ? 1 : 0,
              rows.size());
  std::printf("T12");
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) std::printf(" %.9e", T.linear()(r, c));
  for (int r = 0; r < 3; ++r) std::printf(" %.9e", T.translation()(r));
  std::printf("\n");
  for (const auto &r : rows) std::printf("row %.9e %.9e %.9e\n", r.cost, r.cost_change, r.abs_step);
  std::printf("mask_l ");
  for (bool v : ml) std::printf("%d", v ? 1 : 0);
  std::printf("\nmask_r ");
  if (mr)
    for (bool v : *mr) std::printf("%d", v ? 1 : 0);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) {
    std::printf("usage: test_planar_batch <frames.txt>\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  int B = 0, stereo = 0;
  in >> B >> stereo;
  Options options;
  in >> options.iteration_handle.max_num_iterations >> options.convergence_handle.threshold_step_size >>
      options.convergence_handle.threshold_cost_change >> options.outlier_handle.threshold_huber_loss >>
      options.outlier_handle.threshold_outlier_rejection;
  std::vector<Solver::MonocularFramePlanar3Dof> mono(stereo ? 0 : B);
  std::vector<Solver::StereoFramePlanar3Dof> st(stereo ? B : 0);
  for (int b = 0; b < B; ++b) {
    int n;
    float fx, fy, cx, cy;
    in >> n >> fx >> fy >> cx >> cy;
    const Eigen::Isometry3f T_bc = Read12(in), T_lr = Read12(in), T_wl = Read12(in), T_init = Read12(in);
    std::vector<Eigen::Vector3f> X(n);
    std::vector<Eigen::Vector2f> uvl(n), uvr(n);
    for (int k = 0; k < n; ++k)
      in >> X[k](0) >> X[k](1) >> X[k](2) >> uvl[k](0) >> uvl[k](1) >> uvr[k](0) >> uvr[k](1);
    if (stereo) {
      auto &f = st[b];
      f.world_position_list = X;
      f.matched_left_pixel_list = uvl;
      f.matched_right_pixel_list = uvr;
      f.fx_left = f.fx_right = fx;
      f.fy_left = f.fy_right = fy;
      f.cx_left = f.cx_right = cx;
      f.cy_left = f.cy_right = cy;
      f.base_to_camera_pose = T_bc;
      f.left_to_right_pose = T_lr;
      f.world_to_last_pose = T_wl;
      f.world_to_current_pose = T_init;
    } else {
      auto &f = mono[b];
      f.world_position_list = X;
      f.matched_pixel_list = uvl;
      f.fx = fx;
      f.fy = fy;
      f.cx = cx;
      f.cy = cy;
      f.pose_base_to_camera = T_bc;
      f.pose_world_to_last = T_wl;
      f.pose_world_to_current = T_init;
    }
  }
  if (!in) {
    std::printf("FAIL: could not read %s\n", argv[1]);
    return 2;
  }

  Solver solver;
  bool all;
  if (stereo) {
    all = solver.Solve_Stereo_Planar3Dof_Batch(st, options);
    for (int b = 0; b < B; ++b)
      Print(b, st[b].world_to_current_pose, st[b].success, st[b].summary, st[b].mask_inlier_left,
            &st[b].mask_inlier_right);
  } else {
    all = solver.Solve_Monocular_Planar3Dof_Batch(mono, options);
    for (int b = 0; b < B; ++b)
      Print(b, mono[b].pose_world_to_current, mono[b].success, mono[b].summary, mono[b].mask_inlier, nullptr);
  }
  std::printf("all %d\n", all ? 1 : 0);

  // a size mismatch in any frame throws before any frame is touched
  std::vector<Solver::StereoFramePlanar3Dof> bad(2);
  bad[0].world_position_list.resize(3);
  bad[0].matched_left_pixel_list.resize(3);
  bad[0].matched_right_pixel_list.resize(3);
  bad[1].world_position_list.resize(3);
  bad[1].matched_left_pixel_list.resize(3);
  bad[1].matched_right_pixel_list.resize(2);
  bool thrown = false;
  try {
    solver.Solve_Stereo_Planar3Dof_Batch(bad, options);
  } catch (const std::runtime_error &e) {
    thrown = std::string(e.what()).find("!= right_current_pixel_list.size()") != std::string::npos;
  }
  EXPECT(thrown && bad[0].mask_inlier_left.empty(), "size mismatch must throw before any frame is touched");
  // frames without points: pose kept, success
  std::vector<Solver::MonocularFramePlanar3Dof> empty(2);
  for (auto &f : empty) f.pose_world_to_current = Eigen::Isometry3f::Identity();
  EXPECT(solver.Solve_Monocular_Planar3Dof_Batch(empty, options) && empty[0].success && empty[1].success &&
             empty[0].pose_world_to_current.matrix() == Eigen::Matrix4f::Identity(),
         "n = 0");
  if (g_fail == 0) std::printf("PLANAR BATCH FACADE TEST PASSED\n");
  return g_fail == 0 ? 0 : 1;
}
