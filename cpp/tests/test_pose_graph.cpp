// GPU test of SolvePoseGraph on the C++ facades: pose-graph optimisation over the factors of
// AddRelativePose alone (ba_pgraph_* of include/ba_hip.h).  A chain of 12 poses (pose 0 fixed)
// with drifted start values carries an odometry chain, two loop closures in opposite
// orientations, one pair named twice and one factor whose j is fixed; no camera, point or
// observation is registered.  SolvePoseGraph of FullBundleAdjustmentSolver and of
// FullBundleAdjustmentSolverRefactor in the caller's units must leave behind the caller's
// pointers the poses that ba_pgraph_create + ba_pgraph_solve give when called directly on the
// same arrays in scaled units (the facade's preprocessing restated here), converted as the
// facade's write-back converts, bit for bit, with the same rows in the Summary.  Then, on a
// solver that also holds a finalized full problem with the same factors: SolvePoseGraph,
// ReloadParameterValues and the handle holds the new poses; Solve runs from them.
// Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "ba_hip.h"
#include "core/full_bundle_adjustment_solver.h"
#include "core/full_bundle_adjustment_solver_refactor.h"
#include "eigen3/Eigen/Dense"

using namespace visual_navigation::analytic_solver;
using Rel = FullBundleAdjustmentSolver::RelativePose;
constexpr int kIters = 5, kPoses = 12;

struct Graph {
  std::vector<_BA_Pose> poses;  // start values, world-to-body^-1 as AddPose takes them
  std::vector<_BA_Pose> truth;
};

static Graph MakeGraph(unsigned seed) {
  std::mt19937 gen(seed);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  Graph g;
  g.truth.resize(kPoses);
  for (int j = 0; j < kPoses; ++j) {
    g.truth[j] = _BA_Pose::Identity();
    g.truth[j].translation() = _BA_Point(0.25 * j, 0.02 * j * j, 0.03 * j);
  }
  g.poses = g.truth;
  for (int j = 1; j < kPoses; ++j)
    g.poses[j].translation() += _BA_Point(0.01 * j * U(gen), 0.01 * j * U(gen), 0.01 * j * U(gen));
  return g;
}

static std::vector<Rel> MakeFactors(Graph &g, double sigma) {
  std::vector<std::pair<int, int>> pairs;
  for (int q = 0; q + 1 < kPoses; ++q) pairs.emplace_back(q + 1, q);
  pairs.emplace_back(kPoses - 1, 2);
  pairs.emplace_back(3, 9);
  pairs.emplace_back(9, 3);
  pairs.emplace_back(0, 6);  // j fixed
  const double wgt = 1.0 / (sigma * sigma * 1e-4);
  std::vector<Rel> out;
  for (size_t f = 0; f < pairs.size(); ++f) {
    Rel r;
    r.pose_j = &g.poses[pairs[f].first];
    r.pose_k = &g.poses[pairs[f].second];
    r.measurement = g.truth[pairs[f].first].inverse() * g.truth[pairs[f].second];
    r.measurement.translation() += _BA_Point(0.001, -0.0005 * (1.0 + f), 0.0008);
    for (int a = 0; a < 6; ++a) {
      const double da = a < 3 ? 0.01 : 1.0;
      r.information[6 * a + a] = wgt * da * (a < 3 ? 2e4 : 2e2) * da;
    }
    r.information[6 * 4 + 1] = r.information[6 * 1 + 4] = wgt * 0.01 * 3e2;
    out.push_back(r);
  }
  return out;
}

static void Pack(const _BA_Pose &P, std::vector<double> &v) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) v.push_back(P.linear()(r, c));
  for (int r = 0; r < 3; ++r) v.push_back(P.translation()(r));
}

static ba_options MakeOptions(const Options &o, bool gauss_newton) {
  ba_options c;
  c.threshold_step_size = o.convergence_handle.threshold_step_size;
  c.threshold_cost_change = o.convergence_handle.threshold_cost_change;
  c.threshold_huber_loss = o.outlier_handle.threshold_huber_loss;
  c.threshold_outlier_rejection = o.outlier_handle.threshold_outlier_rejection;
  c.max_num_iterations = o.iteration_handle.max_num_iterations;
  c.initial_lambda = o.trust_region_handle.initial_lambda;
  c.decrease_ratio_lambda = o.trust_region_handle.decrease_ratio_lambda;
  c.increase_ratio_lambda = o.trust_region_handle.increase_ratio_lambda;
  c.gauss_newton = gauss_newton ? 1 : 0;
  return c;
}

#define TRY(expr)                                             \
  do {                                                        \
    if ((expr) != 0) {                                        \
      std::printf("%s failed: %s\n", #expr, ba_last_error()); \
      return false;                                           \
    }                                                         \
  } while (0)

// the facade's preprocessing restated, then the C calls; out: the poses as the write-back
// converts them, T: the scaled T_jw, rows: the iteration rows
static bool Direct(const Graph &g, const std::vector<Rel> &rels, double sigma, const Options &options, bool gn,
                   std::vector<_BA_Pose> *out, std::vector<double> *T, std::vector<ba_iter_info> *rows) {
  const double s = 0.01, inv = 100.0, wgt = 1.0 / (sigma * sigma * s * s);
  std::vector<double> Tp, Z, Om;
  std::vector<uint8_t> pf(g.poses.size(), 0);
  pf[0] = 1;
  std::vector<int32_t> rj, rk;
  for (const _BA_Pose &pose : g.poses) {
    _BA_Pose P = pose.inverse();
    P.translation() = P.translation() * s;
    Pack(P, Tp);
  }
  for (const Rel &r : rels) {
    rj.push_back(static_cast<int32_t>(r.pose_j - &g.poses[0]));
    rk.push_back(static_cast<int32_t>(r.pose_k - &g.poses[0]));
    _BA_Pose Zs = r.measurement;
    Zs.translation() = Zs.translation() * s;
    Pack(Zs, Z);
    for (int rr = 0; rr < 6; ++rr)
      for (int c = 0; c < 6; ++c)
        Om.push_back(((rr < 3 ? inv : 1.0) * r.information[6 * rr + c] * (c < 3 ? inv : 1.0)) / wgt);
  }
  TRY(ba_pgraph_check(static_cast<int>(g.poses.size()), Tp.data(), pf.data(), static_cast<int64_t>(rj.size()), rj.data(),
                      rk.data(), Z.data(), Om.data()));
  ba_handle *h = nullptr;
  TRY(ba_create(&h, 0));
  ba_pgraph *pg = nullptr;
  TRY(ba_pgraph_create(&pg, h, static_cast<int>(g.poses.size()), Tp.data(), pf.data(), static_cast<int64_t>(rj.size()),
                       rj.data(), rk.data(), Z.data(), Om.data()));
  const ba_options o = MakeOptions(options, gn);
  rows->assign(kIters, ba_iter_info());
  int n_iter = 0, converged = 0;
  TRY(ba_pgraph_solve(pg, &o, rows->data(), kIters, &n_iter, &converged));
  T->resize(Tp.size());
  TRY(ba_pgraph_get_poses(pg, T->data()));
  int64_t info[8];
  TRY(ba_pgraph_info(pg, info));
  std::printf("direct (%s): N %lld factors %lld blocks %lld nb %lld, chi2 %.6e -> %.6e\n", gn ? "GN" : "LM",
              (long long)info[0], (long long)info[1], (long long)info[2], (long long)info[3], (*rows)[0].trial_cost,
              (*rows)[kIters - 1].cost);
  ba_pgraph_destroy(pg);
  ba_destroy(h);
  out->clear();
  for (size_t p = 0; p < g.poses.size(); ++p) {
    _BA_Pose T_jw;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T_jw.linear()(r, c) = (*T)[12 * p + 3 * r + c];
      T_jw.translation()(r) = (*T)[12 * p + 9 + r];
    }
    T_jw.translation() *= static_cast<float>(inv);
    out->push_back(p == 0 ? g.poses[0] : T_jw.inverse());
  }
  return n_iter == kIters && info[0] == kPoses - 1 && info[1] == static_cast<int64_t>(rels.size()) && info[7] == 0 &&
         (*rows)[kIters - 1].cost < (*rows)[0].trial_cost * 1e3;
}

static bool SamePoses(const std::vector<_BA_Pose> &a, const std::vector<_BA_Pose> &b) {
  if (a.size() != b.size()) return false;
  for (size_t p = 0; p < a.size(); ++p) {
    std::vector<double> x, y;
    Pack(a[p], x);
    Pack(b[p], y);
    if (std::memcmp(x.data(), y.data(), 12 * sizeof(double)) != 0) return false;
  }
  return true;
}

static bool SameRows(const Summary &s, const std::vector<ba_iter_info> &rows) {
  if (s.GetOptimizationInfoList().size() != rows.size()) return false;
  for (size_t k = 0; k < rows.size(); ++k) {
    const OptimizationInfo &a = s.GetOptimizationInfoList()[k];
    if (a.cost != rows[k].cost || a.damping_term != rows[k].damping_term ||
        static_cast<int>(a.iteration_status) != rows[k].iteration_status || a.abs_step != rows[k].abs_step)
      return false;
  }
  return true;
}

int main() {
  const Graph start = MakeGraph(1);
  const double sigma = 0.7;
  Options options;
  options.solver_type = SolverType::LEVENBERG_MARQUARDT;  // the refactored class selects by it
  options.iteration_handle.max_num_iterations = kIters;
  options.convergence_handle.threshold_step_size = -1.0;
  options.convergence_handle.threshold_cost_change = -1.0;
  options.trust_region_handle.initial_lambda = 1e-4;
  int fail = 0;
  std::vector<_BA_Pose> want_lm, want_gn;
  std::vector<double> T_lm, T_gn;
  std::vector<ba_iter_info> rows_lm, rows_gn;
  {
    Graph g = start;
    const std::vector<Rel> rels = MakeFactors(g, sigma);
    if (!Direct(g, rels, sigma, options, false, &want_lm, &T_lm, &rows_lm)) ++fail;
    if (!Direct(g, rels, sigma, options, true, &want_gn, &T_gn, &rows_gn)) ++fail;
    if (SamePoses(want_lm, g.poses)) ++fail;  // the solve moves the poses
  }
  // ---- FullBundleAdjustmentSolver: no camera, no point, no FinalizeParameters
  {
    Graph g = start;
    const std::vector<Rel> rels = MakeFactors(g, sigma);
    FullBundleAdjustmentSolver s;
    s.SetVerbose(false);
    bool threw = false;
    try {
      s.SolvePoseGraph(options);  // nothing registered
    } catch (const std::runtime_error &) {
      threw = true;
    }
    if (!threw) ++fail;
    for (auto &T : g.poses) s.AddPose(&T);
    s.MakePoseFixed(&g.poses[0]);
    for (const Rel &r : rels) s.AddRelativePose(r, sigma);
    Summary summary;
    if (!s.SolvePoseGraph(options, &summary)) ++fail;
    const bool same = SamePoses(g.poses, want_lm) && SameRows(summary, rows_lm);
    std::printf("FullBundleAdjustmentSolver: %s\n", same ? "same bits" : "DIFFERENT");
    if (!same || summary.IsConverged() || s.GetHandle() != nullptr) ++fail;
  }
  // ---- FullBundleAdjustmentSolverRefactor: solver_type selects LM or Gauss-Newton
  for (int gn = 0; gn < 2; ++gn) {
    Graph g = start;
    const std::vector<Rel> rels = MakeFactors(g, sigma);
    FullBundleAdjustmentSolverRefactor r;
    r.SetVerbose(false);
    for (auto &T : g.poses) r.RegisterWorldToBodyPose(&T);
    r.MakePoseFixed(&g.poses[0]);
    for (const Rel &f : rels) r.AddRelativePose(f, sigma);
    Options o = options;
    o.solver_type = gn ? SolverType::GAUSS_NEWTON : SolverType::LEVENBERG_MARQUARDT;
    Summary summary;
    if (!r.SolvePoseGraph(o, &summary)) ++fail;
    const bool same = SamePoses(g.poses, gn ? want_gn : want_lm) && SameRows(summary, gn ? rows_gn : rows_lm);
    std::printf("FullBundleAdjustmentSolverRefactor (%s): %s\n", gn ? "GN" : "LM", same ? "same bits" : "DIFFERENT");
    if (!same) ++fail;
  }
  // ---- a solver that also holds a finalized full problem with the same factors
  {
    Graph g = start;
    const std::vector<Rel> rels = MakeFactors(g, sigma);
    std::mt19937 gen(5);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    _BA_Camera cam;
    cam.fx = cam.fy = 525.0;
    cam.cx = 320.0;
    cam.cy = 240.0;
    cam.pose_this_to_cam0 = _BA_Pose::Identity();
    std::vector<_BA_Point> points(80);
    for (auto &X : points) X = _BA_Point(1.4 + 1.8 * U(gen), 1.2 + 1.5 * U(gen), 6.0 + 2.0 * U(gen));
    FullBundleAdjustmentSolver s;
    s.SetVerbose(false);
    s.AddCamera(0, cam);
    for (auto &T : g.poses) s.AddPose(&T);
    for (auto &X : points) s.AddPoint(&X);
    s.MakePoseFixed(&g.poses[0]);
    for (int j = 0; j < kPoses; ++j)
      for (size_t i = 0; i < points.size(); ++i) {
        const _BA_Point Xc = g.truth[j].inverse() * points[i];
        s.AddObservation(0, &g.poses[j], &points[i], _BA_Pixel(525.0 * Xc(0) / Xc(2) + 320.0, 525.0 * Xc(1) / Xc(2) + 240.0));
      }
    for (const Rel &r : rels) s.AddRelativePose(r, sigma);
    s.FinalizeParameters();
    std::vector<double> T_before(12 * kPoses), T_after(12 * kPoses);
    if (ba_get_poses(s.GetHandle(), T_before.data()) != 0) ++fail;
    const std::vector<_BA_Point> points_before = points;
    if (!s.SolvePoseGraph(options)) ++fail;
    if (!SamePoses(g.poses, want_lm)) ++fail;  // on the finalized problem's handle: the same bits
    for (size_t i = 0; i < points.size(); ++i)
      if (points[i](0) != points_before[i](0) || points[i](2) != points_before[i](2)) ++fail;  // no point is touched
    s.ReloadParameterValues();
    if (ba_get_poses(s.GetHandle(), T_after.data()) != 0) ++fail;
    double d_new = 0.0, d_old = 0.0;
    for (size_t e = 0; e < T_after.size(); ++e) {
      d_new = std::max(d_new, std::fabs(T_after[e] - T_lm[e]));
      d_old = std::max(d_old, std::fabs(T_after[e] - T_before[e]));
    }
    std::printf("finalized problem after ReloadParameterValues: |T - pose graph| %.3e, |T - before| %.3e\n", d_new, d_old);
    if (!(d_new <= 1e-9) || !(d_old > 1e-6)) ++fail;
    Options full = options;
    full.trust_region_handle.initial_lambda = 100.0;
    full.iteration_handle.max_num_iterations = 2;
    if (!s.Solve(full)) ++fail;
  }
  if (fail) {
    std::printf("%d checks failed\n", fail);
    return 1;
  }
  std::printf("POSE GRAPH FACADE TEST PASSED\n");
  return 0;
}
