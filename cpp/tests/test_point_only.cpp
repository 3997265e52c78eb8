// GPU test of SolvePointsOnly of both C++ classes against ba_point_only called directly
// through include/ba_hip.h on the arrays the facade converts (0.01 scaling, inverted poses,
// landmark-major observations of the non-fixed points): the written points are the bits of
// the direct call times 100, the results are its results, fixed points and every pose stay
// bit for bit; a triangulated point may start as NaN; a Solve follows on the same object.
// Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "ba_hip.h"
#include "core/full_bundle_adjustment_solver.h"
#include "core/full_bundle_adjustment_solver_refactor.h"
#include "eigen3/Eigen/Dense"

using namespace visual_navigation::analytic_solver;

struct Window {
  std::vector<_BA_Camera> cams;
  std::vector<_BA_Pose> poses;
  std::vector<_BA_Point> points;
  std::vector<int> fixed_point;
  struct Obs {
    int c, j, i;
    _BA_Pixel uv;
  };
  std::vector<Obs> obs;
};

static Window MakeWindow(int n_pose, int n_pt, unsigned seed) {
  std::mt19937 gen(seed);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  Window w;
  for (int c = 0; c < 2; ++c) {
    _BA_Camera cam;
    cam.fx = cam.fy = 525.0;
    cam.cx = 320.0;
    cam.cy = 240.0;
    cam.pose_this_to_cam0 = _BA_Pose::Identity();
    cam.pose_this_to_cam0.translation() = _BA_Point(-0.12 * c, 0, 0);
    w.cams.push_back(cam);
  }
  w.poses.resize(n_pose);
  for (int j = 0; j < n_pose; ++j) {
    w.poses[j] = _BA_Pose::Identity();
    w.poses[j].translation() = _BA_Point(0.25 * j, 0.02 * j * j, 0.03 * j);
  }
  std::vector<_BA_Point> Xt(n_pt);
  for (int i = 0; i < n_pt; ++i) Xt[i] = _BA_Point(0.5 + 1.6 * U(gen), 1.0 * U(gen), 6.0 + 2.5 * U(gen));
  // pose-major insertion, half-pixel noise; landmark i is seen by the poses i % 3 .. n_pose - 1
  for (int j = 0; j < n_pose; ++j)
    for (int c = 0; c < 2; ++c)
      for (int i = 0; i < n_pt; ++i) {
        if (j < i % 3) continue;
        const _BA_Point Xc = w.cams[c].pose_this_to_cam0 * (w.poses[j].inverse() * Xt[i]);
        Window::Obs o;
        o.c = c;
        o.j = j;
        o.i = i;
        o.uv = _BA_Pixel(525.0 * Xc(0) / Xc(2) + 320.0 + 0.5 * U(gen), 525.0 * Xc(1) / Xc(2) + 240.0 + 0.5 * U(gen));
        w.obs.push_back(o);
      }
  w.points = Xt;
  w.fixed_point.assign(n_pt, 0);
  w.fixed_point[5] = w.fixed_point[11] = 1;
  for (int i = 0; i < n_pt; ++i)
    if (!w.fixed_point[i]) w.points[i] += _BA_Point(0.3 * U(gen), 0.3 * U(gen), 0.6 * U(gen));
  w.points[7] = _BA_Point::Constant(std::numeric_limits<double>::quiet_NaN());  // triangulated
  return w;
}

static bool SameBits(const _BA_Point &a, const _BA_Point &b) { return std::memcmp(a.data(), b.data(), 24) == 0; }
static bool Finite(const _BA_Point &a) { return std::isfinite(a(0)) && std::isfinite(a(1)) && std::isfinite(a(2)); }
static bool SameBits(const _BA_Pose &a, const _BA_Pose &b) {
  const auto A = a.matrix(), B = b.matrix();
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      const double x = A(r, c), y = B(r, c);
      if (std::memcmp(&x, &y, 8)) return false;
    }
  return true;
}

template <class Solver>
static void Register(Solver &s, Window &w);

template <>
void Register<FullBundleAdjustmentSolver>(FullBundleAdjustmentSolver &s, Window &w) {
  s.SetVerbose(false);
  for (size_t c = 0; c < w.cams.size(); ++c) s.AddCamera(static_cast<int>(c), w.cams[c]);
  for (auto &T : w.poses) s.AddPose(&T);
  for (auto &X : w.points) s.AddPoint(&X);
  s.MakePoseFixed(&w.poses[0]);
  for (size_t i = 0; i < w.points.size(); ++i)
    if (w.fixed_point[i]) s.MakePointFixed(&w.points[i]);
  for (const auto &o : w.obs) s.AddObservation(o.c, &w.poses[o.j], &w.points[o.i], o.uv);
}

template <>
void Register<FullBundleAdjustmentSolverRefactor>(FullBundleAdjustmentSolverRefactor &s, Window &w) {
  s.SetVerbose(false);
  for (size_t c = 0; c < w.cams.size(); ++c) {
    OptimizerCamera cam;
    cam.fx = w.cams[c].fx;
    cam.fy = w.cams[c].fy;
    cam.cx = w.cams[c].cx;
    cam.cy = w.cams[c].cy;
    cam.camera_to_body_pose = w.cams[c].pose_this_to_cam0;
    s.RegisterCamera(static_cast<int>(c), cam);
  }
  for (auto &T : w.poses) s.RegisterWorldToBodyPose(&T);
  for (auto &X : w.points) s.RegisterWorldPoint(&X);
  s.MakePoseFixed(&w.poses[0]);
  for (size_t i = 0; i < w.points.size(); ++i)
    if (w.fixed_point[i]) s.MakePointFixed(&w.points[i]);
  for (const auto &o : w.obs) s.AddObservation(o.c, &w.poses[o.j], &w.points[o.i], o.uv);
}

// the direct call in scaled units on the same window: X (non-fixed points, registration order)
static int Direct(const Window &w, const ba_options &opt, std::vector<double> *X, std::vector<ba_point_result> *res,
                  std::vector<int> *sel) {
  const double s = 0.01;
  std::vector<double> intr, T_cj, T;
  for (const auto &c : w.cams) {
    intr.insert(intr.end(), {c.fx * s, c.fy * s, c.cx * s, c.cy * s});
    _BA_Pose P = c.pose_this_to_cam0;
    P.translation() *= s;
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) T_cj.push_back(P.linear()(r, k));
    for (int r = 0; r < 3; ++r) T_cj.push_back(P.translation()(r));
  }
  for (const auto &pose : w.poses) {
    _BA_Pose P = pose.inverse();
    P.translation() = P.translation() * s;
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) T.push_back(P.linear()(r, k));
    for (int r = 0; r < 3; ++r) T.push_back(P.translation()(r));
  }
  std::vector<int> new_of(w.points.size(), -1);
  sel->clear();
  for (size_t i = 0; i < w.points.size(); ++i)
    if (!w.fixed_point[i]) {
      new_of[i] = static_cast<int>(sel->size());
      sel->push_back(static_cast<int>(i));
    }
  const int n_pt = static_cast<int>(sel->size());
  std::vector<int64_t> off(n_pt + 1, 0);
  std::vector<int32_t> oc, op;
  std::vector<double> uv;
  std::vector<uint8_t> tri(n_pt, 0);
  X->clear();
  for (int t = 0; t < n_pt; ++t) {
    const int i = (*sel)[t];
    for (const auto &o : w.obs)
      if (o.i == i) {
        oc.push_back(o.c);
        op.push_back(o.j);
        uv.push_back(o.uv(0) * s);
        uv.push_back(o.uv(1) * s);
      }
    off[t + 1] = static_cast<int64_t>(oc.size());
    const _BA_Point Xs = w.points[i] * s;
    for (int r = 0; r < 3; ++r) X->push_back(Xs(r));
    tri[t] = i == 7;
  }
  res->assign(n_pt, ba_point_result());
  ba_handle *h = nullptr;
  if (ba_create(&h, 0) != 0) return -1;
  const int rc = ba_point_only(h, 2, intr.data(), T_cj.data(), static_cast<int>(w.poses.size()), T.data(), n_pt,
                               off.data(), oc.data(), op.data(), uv.data(), tri.data(), X->data(), &opt, nullptr, 0,
                               res->data());
  ba_destroy(h);
  return rc;
}

template <class Solver>
static int RunClass(const char *name, const Window &base, Options options, bool gauss_newton) {
  int fail = 0;
  ba_options o;
  o.threshold_step_size = options.convergence_handle.threshold_step_size;
  o.threshold_cost_change = options.convergence_handle.threshold_cost_change;
  o.threshold_huber_loss = options.outlier_handle.threshold_huber_loss;
  o.threshold_outlier_rejection = options.outlier_handle.threshold_outlier_rejection;
  o.max_num_iterations = options.iteration_handle.max_num_iterations;
  o.initial_lambda = options.trust_region_handle.initial_lambda;
  o.decrease_ratio_lambda = options.trust_region_handle.decrease_ratio_lambda;
  o.increase_ratio_lambda = options.trust_region_handle.increase_ratio_lambda;
  o.gauss_newton = gauss_newton ? 1 : 0;
  std::vector<double> X;
  std::vector<ba_point_result> want;
  std::vector<int> sel;
  if (Direct(base, o, &X, &want, &sel) != 0) {
    std::printf("%s: the direct call failed: %s\n", name, ba_last_error());
    return 1;
  }
  Window w = base;
  Solver s;
  Register(s, w);
  std::vector<typename Solver::PointOnlyResult> got;
  const bool ok = s.SolvePointsOnly(options, &got, {&w.points[7]});
  if (!ok || got.size() != sel.size()) ++fail;
  int moved = 0, iters = 0;
  for (size_t t = 0; t < sel.size() && t < got.size(); ++t) {
    const int i = sel[t];
    const ba_point_result &r = want[t];
    if (got[t].point != &w.points[i] || got[t].status != 0 || r.status != 0) ++fail;
    if (got[t].n_iter != r.n_iter || got[t].converged != r.converged || got[t].n_behind != r.n_behind ||
        got[t].dropped_pivots != r.dropped_pivots)
      ++fail;
    if (std::memcmp(&got[t].cost0, &r.cost0, 8) || std::memcmp(&got[t].cost, &r.cost, 8)) ++fail;
    const _BA_Point Xu = _BA_Point(X[3 * t], X[3 * t + 1], X[3 * t + 2]) * 100.0;
    if (!SameBits(Xu, w.points[i])) ++fail;
    if (!SameBits(w.points[i], base.points[i])) ++moved;
    iters += r.n_iter;
  }
  for (size_t i = 0; i < w.points.size(); ++i)
    if (w.fixed_point[i] && !SameBits(w.points[i], base.points[i])) ++fail;
  for (size_t j = 0; j < w.poses.size(); ++j)
    if (!SameBits(w.poses[j], base.poses[j])) ++fail;
  if (!Finite(w.points[7])) ++fail;
  if (moved < static_cast<int>(sel.size()) - 1 || iters < static_cast<int>(sel.size())) ++fail;
  // an unknown and a fixed pointer are refused
  _BA_Point stranger(0, 0, 1);
  for (_BA_Point *bad : {&stranger, &w.points[5]}) {
    bool threw = false;
    try {
      s.SolvePointsOnly(options, nullptr, {bad});
    } catch (const std::runtime_error &) {
      threw = true;
    }
    if (!threw) ++fail;
  }
  // a Solve follows on the same object, from the new points
  Options so = options;
  so.iteration_handle.max_num_iterations = 3;
  Summary summary;
  s.Solve(so, &summary);
  if (summary.GetOptimizationInfoList().empty()) ++fail;
  for (const auto &X3 : w.points)
    if (!Finite(X3)) ++fail;
  // ... and a second point-only solve on the finalized object
  if (!s.SolvePointsOnly(options, &got)) ++fail;
  std::printf("%s (%s): %zu points, %d iterations in all, %d moved, failures %d\n", name,
              gauss_newton ? "Gauss-Newton" : "LM", sel.size(), iters, moved, fail);
  return fail;
}

int main() {
  const Window base = MakeWindow(6, 23, 4);
  Options options;
  options.iteration_handle.max_num_iterations = 20;
  options.solver_type = SolverType::LEVENBERG_MARQUARDT;
  int fail = RunClass<FullBundleAdjustmentSolver>("FullBundleAdjustmentSolver", base, options, false);
  fail += RunClass<FullBundleAdjustmentSolverRefactor>("FullBundleAdjustmentSolverRefactor", base, options, false);
  options.solver_type = SolverType::GAUSS_NEWTON;
  options.iteration_handle.max_num_iterations = 5;
  fail += RunClass<FullBundleAdjustmentSolverRefactor>("FullBundleAdjustmentSolverRefactor", base, options, true);
  std::printf(fail ? "POINT ONLY FACADE TEST FAILED (%d)\n" : "POINT ONLY FACADE TEST PASSED\n", fail);
  return fail ? 1 : 0;
}
