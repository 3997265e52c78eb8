// GPU test of FullBundleAdjustmentSolver::SolveBatch: three small windows (stereo 5 poses,
// mono 4 poses, stereo 6 poses with a fixed point) are solved once by one Solve per
// solver object and once by ONE SolveBatch over three identical objects; poses, points
// and Summary rows must agree to the tolerances of the Python parity tests (status
// identical, lambda 1e-12, cost 1e-7, parameters 1e-6 relative), and fixed objects stay
// bit for bit untouched.  Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "core/full_bundle_adjustment_solver.h"
#include "eigen3/Eigen/Dense"

using namespace visual_navigation::analytic_solver;

struct Window {
  std::vector<_BA_Camera> cams;
  std::vector<_BA_Pose> poses;
  std::vector<_BA_Point> points;
  std::vector<int> fixed_pose, fixed_point;
  struct Obs {
    int c, j, i;
    _BA_Pixel uv;
  };
  std::vector<Obs> obs;
};

static Window MakeWindow(int n_pose, int n_pt, bool stereo, unsigned seed, int fixed_point) {
  std::mt19937 gen(seed);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  Window w;
  const int n_cam = stereo ? 2 : 1;
  for (int c = 0; c < n_cam; ++c) {
    _BA_Camera cam;
    cam.fx = cam.fy = 525.0;
    cam.cx = 320.0;
    cam.cy = 240.0;
    cam.pose_this_to_cam0 = _BA_Pose::Identity();
    cam.pose_this_to_cam0.translation() = _BA_Point(-0.12 * c, 0, 0);  // body -> camera c
    w.cams.push_back(cam);
  }
  std::vector<_BA_Pose> truth(n_pose);
  for (int j = 0; j < n_pose; ++j) {
    truth[j] = _BA_Pose::Identity();
    truth[j].translation() = _BA_Point(0.25 * j, 0.02 * j * j, 0.03 * j);
  }
  std::vector<_BA_Point> Xt(n_pt);
  for (int i = 0; i < n_pt; ++i) Xt[i] = _BA_Point(0.5 + 1.6 * U(gen), 1.0 * U(gen), 6.0 + 2.5 * U(gen));
  for (int j = 0; j < n_pose; ++j)
    for (int c = 0; c < n_cam; ++c)
      for (int i = 0; i < n_pt; ++i) {
        const _BA_Point Xc = w.cams[c].pose_this_to_cam0 * (truth[j].inverse() * Xt[i]);
        Window::Obs o;
        o.c = c;
        o.j = j;
        o.i = i;
        o.uv = _BA_Pixel(525.0 * Xc(0) / Xc(2) + 320.0, 525.0 * Xc(1) / Xc(2) + 240.0);
        w.obs.push_back(o);
      }
  w.poses = truth;
  w.fixed_pose.assign(n_pose, 0);
  w.fixed_pose[0] = w.fixed_pose[1] = 1;
  for (int j = 2; j < n_pose; ++j) w.poses[j].translation() += _BA_Point(0.04 * U(gen), 0.04 * U(gen), 0.04 * U(gen));
  w.points = Xt;
  w.fixed_point.assign(n_pt, 0);
  for (int i = 0; i < n_pt; ++i)
    if (i == fixed_point)
      w.fixed_point[i] = 1;
    else
      w.points[i] += _BA_Point(0.15 * U(gen), 0.15 * U(gen), 0.15 * U(gen));
  return w;
}

static void Register(FullBundleAdjustmentSolver &s, Window &w) {
  s.SetVerbose(false);
  for (size_t c = 0; c < w.cams.size(); ++c) s.AddCamera(static_cast<int>(c), w.cams[c]);
  for (auto &T : w.poses) s.AddPose(&T);
  for (auto &X : w.points) s.AddPoint(&X);
  for (size_t j = 0; j < w.poses.size(); ++j)
    if (w.fixed_pose[j]) s.MakePoseFixed(&w.poses[j]);
  for (size_t i = 0; i < w.points.size(); ++i)
    if (w.fixed_point[i]) s.MakePointFixed(&w.points[i]);
  for (const auto &o : w.obs) s.AddObservation(o.c, &w.poses[o.j], &w.points[o.i], o.uv);
}

static double Rel(double a, double b, double scale) { return std::fabs(a - b) / scale; }

int main() {
  const std::vector<Window> base = {MakeWindow(5, 30, true, 1, -1), MakeWindow(4, 26, false, 2, -1),
                                    MakeWindow(6, 34, true, 3, 7)};
  Options options;
  options.iteration_handle.max_num_iterations = 6;
  options.convergence_handle.threshold_step_size = 0.0;
  options.convergence_handle.threshold_cost_change = 0.0;
  std::vector<Window> one = base, many = base;
  std::vector<Summary> sum_one(base.size()), sum_many;
  for (size_t k = 0; k < base.size(); ++k) {
    FullBundleAdjustmentSolver s;
    Register(s, one[k]);
    s.Solve(options, &sum_one[k]);
  }
  std::vector<std::unique_ptr<FullBundleAdjustmentSolver>> own;
  std::vector<FullBundleAdjustmentSolver *> ptrs;
  for (size_t k = 0; k < base.size(); ++k) {
    own.emplace_back(new FullBundleAdjustmentSolver());
    Register(*own.back(), many[k]);
    ptrs.push_back(own.back().get());
  }
  int fail = FullBundleAdjustmentSolver::SolveBatch(ptrs, options, &sum_many) ? 0 : 1;
  if (sum_many.size() != base.size()) ++fail;
  for (size_t k = 0; k < base.size() && !fail; ++k) {
    double ep = 0, ex = 0, moved = 0;
    for (size_t j = 0; j < base[k].poses.size(); ++j)
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
          const double a = many[k].poses[j].matrix()(r, c), b = one[k].poses[j].matrix()(r, c);
          ep = std::max(ep, Rel(a, b, 1.0));
          if (base[k].fixed_pose[j] && a != base[k].poses[j].matrix()(r, c)) ++fail;
        }
    for (size_t i = 0; i < base[k].points.size(); ++i)
      for (int r = 0; r < 3; ++r) {
        ex = std::max(ex, Rel(many[k].points[i](r), one[k].points[i](r), 8.0));
        moved = std::max(moved, std::fabs(many[k].points[i](r) - base[k].points[i](r)));
        if (base[k].fixed_point[i] && many[k].points[i](r) != base[k].points[i](r)) ++fail;
      }
    const auto &ra = sum_many[k].GetOptimizationInfoList(), &rb = sum_one[k].GetOptimizationInfoList();
    if (ra.size() != 6 || rb.size() != 6) ++fail;
    double ec = 0, el = 0;
    for (size_t t = 0; t < ra.size() && t < rb.size(); ++t) {
      if (ra[t].iteration_status != rb[t].iteration_status) ++fail;
      ec = std::max(ec, Rel(ra[t].cost, rb[t].cost, std::fabs(rb[t].cost)));
      el = std::max(el, Rel(ra[t].damping_term, rb[t].damping_term, std::fabs(rb[t].damping_term)));
    }
    std::printf("window %zu: max rel err pose %.2e point %.2e cost %.2e lambda %.2e, points moved %.3f\n", k, ep, ex, ec,
                el, moved);
    if (!(ep < 1e-6 && ex < 1e-6 && ec < 1e-7 && el < 1e-12) || !(moved > 1e-3)) ++fail;
  }
  std::printf(fail ? "FULL BATCH FACADE TEST FAILED (%d)\n" : "FULL BATCH FACADE TEST PASSED\n", fail);
  return fail ? 1 : 0;
}
