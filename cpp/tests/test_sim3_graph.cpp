// GPU test of AddRelativeSim3 / SolveSim3Graph on the C++ facades: the 7-DoF loop closing of a
// monocular map (ba_sim3_* of include/ba_hip.h).  A loop of 40 rigid keyframes on a circle whose
// map drifted in scale by c_q = exp(0.003 q), three landmarks anchored to each keyframe.  The
// start is the rigid odometry of the drifted map; the chain factors are the exact similarities
// (R_E, c_q t_E, c_q / c_(q-1)), three closures join the ends, so the zero-residual optimum is
// S_q = (R_q, c_q t_q, c_q), whose rigid form is the truth.
// SolveSim3Graph of FullBundleAdjustmentSolver and of FullBundleAdjustmentSolverRefactor in the
// caller's units must leave behind the caller's pointers what ba_sim3_create + ba_sim3_solve give
// when called directly on the same arrays in scaled units (the facade's preprocessing restated
// here), bit for bit, with the same rows in the Summary and the same scales.  The written-back
// poses are rigid, every anchored point reprojects into its anchor keyframe where it did before
// (1e-9 px), the scales recover the injected drift (1e-8, the bound of the noise-free scenes),
// and SolvePoseGraph on a solver that holds both kinds of factor ignores the Sim(3) ones.
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
using Sim = FullBundleAdjustmentSolver::RelativeSim3;
using Rel = FullBundleAdjustmentSolver::RelativePose;
constexpr int kIters = 7, kPoses = 40, kPerKf = 3;
constexpr double kFx = 500.0, kCx = 320.0, kCy = 240.0;

struct Scene {
  std::vector<_BA_Pose> poses;   // start values as AddPose takes them
  std::vector<_BA_Pose> truth;   // T_wj
  std::vector<double> scale;     // c_q
  std::vector<_BA_Point> points;
  std::vector<int> anchors;
};

static Scene MakeScene() {
  const double kPi = 3.14159265358979323846;
  Scene sc;
  for (int q = 0; q < kPoses; ++q) {
    const double a = 2.0 * kPi * q / kPoses;
    _BA_Pose T = _BA_Pose::Identity();
    T.linear()(0, 0) = std::cos(a);
    T.linear()(0, 2) = std::sin(a);
    T.linear()(2, 0) = -std::sin(a);
    T.linear()(2, 2) = std::cos(a);
    T.translation() = _BA_Point(5.0 * std::cos(a), 0.1 * std::sin(3.0 * a), 5.0 * std::sin(a));
    sc.truth.push_back(T);
    sc.scale.push_back(std::exp(0.003 * q));
  }
  std::vector<_BA_Pose> start_jw(1, sc.truth[0].inverse());
  for (int q = 1; q < kPoses; ++q) {
    _BA_Pose E = sc.truth[q].inverse() * sc.truth[q - 1];  // T_jw(q) T_jw(q-1)^-1
    E.translation() = E.translation() * sc.scale[q];
    start_jw.push_back(E * start_jw.back());
  }
  for (const _BA_Pose &T : start_jw) sc.poses.push_back(T.inverse());
  std::mt19937 gen(31);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  for (int q = 0; q < kPoses; ++q)
    for (int i = 0; i < kPerKf; ++i) {
      sc.points.push_back(sc.poses[q] * _BA_Point(U(gen), U(gen), 4.0 + 2.0 * U(gen)));
      sc.anchors.push_back(q);
    }
  return sc;
}

static std::vector<std::pair<int, int>> Pairs() {
  std::vector<std::pair<int, int>> pairs;
  for (int q = 1; q < kPoses; ++q) pairs.emplace_back(q, q - 1);
  pairs.emplace_back(kPoses - 1, 0);  // k fixed
  pairs.emplace_back(kPoses - 2, 1);
  pairs.emplace_back(2, kPoses - 3);
  return pairs;
}

static std::vector<Sim> MakeSim3(Scene &sc, double sigma) {
  const double wgt = 1.0 / (sigma * sigma * 1e-4);
  std::vector<Sim> out;
  const auto pairs = Pairs();
  for (size_t f = 0; f < pairs.size(); ++f) {
    const int j = pairs[f].first, k = pairs[f].second;
    const _BA_Pose E = sc.truth[j].inverse() * sc.truth[k];
    Sim r;
    r.pose_j = &sc.poses[j];
    r.pose_k = &sc.poses[k];
    for (int a = 0; a < 3; ++a) {
      for (int c = 0; c < 3; ++c) r.measurement[4 * a + c] = (sc.scale[j] / sc.scale[k]) * E.linear()(a, c);
      r.measurement[4 * a + 3] = sc.scale[j] * E.translation()(a);
    }
    for (int a = 0; a < 7; ++a) {
      const double da = a < 3 ? 0.01 : 1.0;
      r.information[7 * a + a] = wgt * da * (a < 3 ? 2e4 : (a < 6 ? 2e2 : 1e2)) * da * (1.0 + 0.1 * (f % 3));
    }
    r.information[7 * 4 + 1] = r.information[7 * 1 + 4] = wgt * 0.01 * 3e2;
    r.information[7 * 6 + 2] = r.information[7 * 2 + 6] = wgt * 0.01 * 1e2;
    out.push_back(r);
  }
  return out;
}

// rigid odometry of the drifted map, slightly off: the factors of SolvePoseGraph
static std::vector<Rel> MakeSe3(Scene &sc, double sigma) {
  const double wgt = 1.0 / (sigma * sigma * 1e-4);
  std::vector<Rel> out;
  for (int q = 1; q < kPoses; ++q) {
    Rel r;
    r.pose_j = &sc.poses[q];
    r.pose_k = &sc.poses[q - 1];
    r.measurement = sc.poses[q].inverse() * sc.poses[q - 1];
    r.measurement.translation() += _BA_Point(0.01, -0.005, 0.008);
    for (int a = 0; a < 6; ++a) {
      const double da = a < 3 ? 0.01 : 1.0;
      r.information[6 * a + a] = wgt * da * (a < 3 ? 2e4 : 2e2) * da;
    }
    out.push_back(r);
  }
  return out;
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

struct Result {
  std::vector<_BA_Pose> poses;
  std::vector<_BA_Point> points;
  std::vector<double> scales;
  std::vector<ba_iter_info> rows;
};

// the facade's preprocessing restated, then the C calls, then its write-back restated
static bool Direct(const Scene &sc, const std::vector<Sim> &rels, double sigma, const Options &options, bool gn,
                   Result *out) {
  const double s = 0.01, inv = 100.0, wgt = 1.0 / (sigma * sigma * s * s);
  const size_t n = sc.poses.size();
  std::vector<double> S, Z, Om;
  std::vector<uint8_t> pf(n, 0);
  pf[0] = 1;
  std::vector<int32_t> rj, rk;
  for (const _BA_Pose &pose : sc.poses) {
    _BA_Pose P = pose.inverse();
    P.translation() = P.translation() * s;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) S.push_back(P.linear()(r, c));
    for (int r = 0; r < 3; ++r) S.push_back(P.translation()(r));
    S.push_back(1.0);
  }
  for (const Sim &r : rels) {
    rj.push_back(static_cast<int32_t>(r.pose_j - &sc.poses[0]));
    rk.push_back(static_cast<int32_t>(r.pose_k - &sc.poses[0]));
    const double *M = r.measurement;
    const double det = M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) +
                       M[2] * (M[4] * M[9] - M[5] * M[8]);
    const double sz = std::cbrt(det);
    for (int a = 0; a < 3; ++a)
      for (int c = 0; c < 3; ++c) Z.push_back(M[4 * a + c] / sz);
    for (int a = 0; a < 3; ++a) Z.push_back(M[4 * a + 3] * s);
    Z.push_back(sz);
    for (int a = 0; a < 7; ++a)
      for (int c = 0; c < 7; ++c) Om.push_back(((a < 3 ? inv : 1.0) * r.information[7 * a + c] * (c < 3 ? inv : 1.0)) / wgt);
  }
  TRY(ba_sim3_check(static_cast<int>(n), S.data(), pf.data(), static_cast<int64_t>(rj.size()), rj.data(), rk.data(),
                    Z.data(), Om.data()));
  ba_handle *h = nullptr;
  TRY(ba_create(&h, 0));
  ba_sim3 *g = nullptr;
  TRY(ba_sim3_create(&g, h, static_cast<int>(n), S.data(), pf.data(), static_cast<int64_t>(rj.size()), rj.data(),
                     rk.data(), Z.data(), Om.data()));
  const ba_options o = MakeOptions(options, gn);
  out->rows.assign(kIters, ba_iter_info());
  int n_iter = 0, converged = 0;
  TRY(ba_sim3_solve(g, &o, out->rows.data(), kIters, &n_iter, &converged));
  std::vector<double> Sn(S.size());
  TRY(ba_sim3_get_poses(g, Sn.data()));
  int64_t info[9];
  TRY(ba_sim3_info(g, info));
  std::printf("direct (%s): N %lld factors %lld blocks %lld nb %lld tiles %lld, chi2 %.6e -> %.6e\n", gn ? "GN" : "LM",
              (long long)info[0], (long long)info[1], (long long)info[2], (long long)info[3], (long long)info[4],
              out->rows[0].trial_cost, out->rows[kIters - 1].cost);
  ba_sim3_destroy(g);
  ba_destroy(h);
  out->poses.clear();
  out->scales.clear();
  for (size_t p = 0; p < n; ++p) {
    const double sp = Sn[13 * p + 12];
    _BA_Pose T_jw;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T_jw.linear()(r, c) = Sn[13 * p + 3 * r + c];
      T_jw.translation()(r) = Sn[13 * p + 9 + r] / sp;
    }
    T_jw.translation() *= inv;
    out->poses.push_back(p == 0 ? sc.poses[0] : T_jw.inverse());
    out->scales.push_back(sp);
  }
  out->points = sc.points;
  for (size_t q = 0; q < sc.points.size(); ++q) {
    const double *So = &S[13 * static_cast<size_t>(sc.anchors[q])], *Sw = &Sn[13 * static_cast<size_t>(sc.anchors[q])];
    const _BA_Point X = sc.points[q] * s;
    double Y[3], Xn[3];
    for (int r = 0; r < 3; ++r)
      Y[r] = ((So[3 * r] * X(0) + So[3 * r + 1] * X(1) + So[3 * r + 2] * X(2) + So[9 + r]) - Sw[9 + r]) / Sw[12];
    for (int r = 0; r < 3; ++r) Xn[r] = Sw[r] * Y[0] + Sw[3 + r] * Y[1] + Sw[6 + r] * Y[2];
    out->points[q] = _BA_Point(Xn[0], Xn[1], Xn[2]) * inv;
  }
  return n_iter == kIters && info[0] == kPoses - 1 && info[1] == static_cast<int64_t>(rels.size()) && info[7] == 0 &&
         out->rows[kIters - 1].cost < 1e-6 * out->rows[0].trial_cost;
}

static bool SamePoses(const std::vector<_BA_Pose> &a, const std::vector<_BA_Pose> &b) {
  if (a.size() != b.size()) return false;
  for (size_t p = 0; p < a.size(); ++p)
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c)
        if (std::memcmp(&a[p].linear()(r, c), &b[p].linear()(r, c), sizeof(double)) != 0) return false;
      if (std::memcmp(&a[p].translation()(r), &b[p].translation()(r), sizeof(double)) != 0) return false;
    }
  return true;
}

static bool SamePoints(const std::vector<_BA_Point> &a, const std::vector<_BA_Point> &b) {
  if (a.size() != b.size()) return false;
  for (size_t q = 0; q < a.size(); ++q)
    for (int r = 0; r < 3; ++r)
      if (std::memcmp(&a[q](r), &b[q](r), sizeof(double)) != 0) return false;
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

static void Project(const _BA_Pose &pose, const _BA_Point &X, double uv[2]) {
  const _BA_Point Xc = pose.inverse() * X;
  uv[0] = kFx * Xc(0) / Xc(2) + kCx;
  uv[1] = kFx * Xc(1) / Xc(2) + kCy;
}

// rigid to 1e-12, anchored reprojections unchanged to 1e-9 px, scales on the injected drift to 1e-8
static bool Geometry(const Scene &before, const Scene &after, const std::vector<double> &scales) {
  double rigid = 0.0, shift = 0.0, ds = 0.0;
  for (size_t p = 0; p < after.poses.size(); ++p) {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        double v = 0.0;
        for (int m = 0; m < 3; ++m) v += after.poses[p].linear()(m, r) * after.poses[p].linear()(m, c);
        rigid = std::max(rigid, std::fabs(v - (r == c ? 1.0 : 0.0)));
      }
    ds = std::max(ds, std::fabs(std::log(scales[p] / before.scale[p])));
  }
  for (size_t q = 0; q < after.points.size(); ++q) {
    double a[2], b[2];
    Project(before.poses[before.anchors[q]], before.points[q], a);
    Project(after.poses[after.anchors[q]], after.points[q], b);
    shift = std::max(shift, std::max(std::fabs(a[0] - b[0]), std::fabs(a[1] - b[1])));
  }
  std::printf("  |R^T R - I| %.2e, reprojection shift %.2e px, |log(scale / injected)| %.2e\n", rigid, shift, ds);
  return rigid <= 1e-12 && shift <= 1e-9 && ds <= 1e-8;
}

int main() {
  const Scene start = MakeScene();
  const double sigma = 0.7;
  Options options;
  options.solver_type = SolverType::LEVENBERG_MARQUARDT;  // the refactored class selects by it
  options.iteration_handle.max_num_iterations = kIters;
  options.convergence_handle.threshold_step_size = -1.0;
  options.convergence_handle.threshold_cost_change = -1.0;
  options.trust_region_handle.initial_lambda = 1e-4;
  int fail = 0;
  Result want_lm, want_gn;
  {
    Scene sc = start;
    const std::vector<Sim> rels = MakeSim3(sc, sigma);
    if (!Direct(sc, rels, sigma, options, false, &want_lm)) ++fail;
    if (!Direct(sc, rels, sigma, options, true, &want_gn)) ++fail;
    if (SamePoses(want_lm.poses, sc.poses)) ++fail;  // the solve moves the poses
  }
  // ---- FullBundleAdjustmentSolver: no camera, no observation, no FinalizeParameters
  {
    Scene sc = start;
    const std::vector<Sim> rels = MakeSim3(sc, sigma);
    FullBundleAdjustmentSolver s;
    s.SetVerbose(false);
    bool threw = false;
    try {
      s.SolveSim3Graph(options);  // nothing registered
    } catch (const std::runtime_error &) {
      threw = true;
    }
    if (!threw) ++fail;
    for (auto &T : sc.poses) s.AddPose(&T);
    for (auto &X : sc.points) s.AddPoint(&X);
    s.MakePoseFixed(&sc.poses[0]);
    for (const Sim &r : rels) s.AddRelativeSim3(r, sigma);
    Summary summary;
    std::vector<double> scales;
    if (!s.SolveSim3Graph(options, &summary, &sc.anchors, &scales)) ++fail;
    const bool same = SamePoses(sc.poses, want_lm.poses) && SamePoints(sc.points, want_lm.points) &&
                      SameRows(summary, want_lm.rows) && scales == want_lm.scales;
    std::printf("FullBundleAdjustmentSolver: %s\n", same ? "same bits" : "DIFFERENT");
    if (!same || summary.IsConverged() || s.GetHandle() != nullptr) ++fail;
    if (!Geometry(start, sc, scales) || scales[0] != 1.0) ++fail;
  }
  // ---- FullBundleAdjustmentSolverRefactor: solver_type selects LM or Gauss-Newton
  for (int gn = 0; gn < 2; ++gn) {
    Scene sc = start;
    const std::vector<Sim> rels = MakeSim3(sc, sigma);
    FullBundleAdjustmentSolverRefactor r;
    r.SetVerbose(false);
    for (auto &T : sc.poses) r.RegisterWorldToBodyPose(&T);
    for (auto &X : sc.points) r.RegisterWorldPoint(&X);
    r.MakePoseFixed(&sc.poses[0]);
    for (const Sim &f : rels) r.AddRelativeSim3(f, sigma);
    Options o = options;
    o.solver_type = gn ? SolverType::GAUSS_NEWTON : SolverType::LEVENBERG_MARQUARDT;
    Summary summary;
    std::vector<double> scales;
    if (!r.SolveSim3Graph(o, &summary, &sc.anchors, &scales)) ++fail;
    const Result &want = gn ? want_gn : want_lm;
    const bool same = SamePoses(sc.poses, want.poses) && SamePoints(sc.points, want.points) &&
                      SameRows(summary, want.rows) && scales == want.scales;
    std::printf("FullBundleAdjustmentSolverRefactor (%s): %s\n", gn ? "GN" : "LM", same ? "same bits" : "DIFFERENT");
    if (!same) ++fail;
    if (!Geometry(start, sc, scales)) ++fail;
  }
  // ---- without anchors no point moves; each solve uses its own kind of factor
  {
    Scene a = start, b = start, c = start;
    const std::vector<Sim> sim_a = MakeSim3(a, sigma), sim_c = MakeSim3(c, sigma);
    const std::vector<Rel> se3_a = MakeSe3(a, sigma), se3_b = MakeSe3(b, sigma);
    FullBundleAdjustmentSolver both, only_se3, only_sim3;
    for (FullBundleAdjustmentSolver *s : {&both, &only_se3, &only_sim3}) s->SetVerbose(false);
    for (auto &T : a.poses) both.AddPose(&T);
    for (auto &T : b.poses) only_se3.AddPose(&T);
    for (auto &T : c.poses) only_sim3.AddPose(&T);
    for (auto &X : c.points) only_sim3.AddPoint(&X);
    both.MakePoseFixed(&a.poses[0]);
    only_se3.MakePoseFixed(&b.poses[0]);
    only_sim3.MakePoseFixed(&c.poses[0]);
    for (const Sim &f : sim_a) both.AddRelativeSim3(f, sigma);
    for (const Rel &f : se3_a) both.AddRelativePose(f, sigma);
    for (const Rel &f : se3_b) only_se3.AddRelativePose(f, sigma);
    for (const Sim &f : sim_c) only_sim3.AddRelativeSim3(f, sigma);
    if (!both.SolvePoseGraph(options) || !only_se3.SolvePoseGraph(options)) ++fail;
    const bool ignored = SamePoses(a.poses, b.poses) && !SamePoses(a.poses, start.poses);
    std::printf("SolvePoseGraph beside Sim(3) factors: %s\n", ignored ? "same bits" : "DIFFERENT");
    if (!ignored) ++fail;
    bool threw = false;
    try {
      only_se3.SolveSim3Graph(options);  // no Sim(3) factor
    } catch (const std::runtime_error &) {
      threw = true;
    }
    if (!threw) ++fail;
    if (!only_sim3.SolveSim3Graph(options)) ++fail;
    if (!SamePoses(c.poses, want_lm.poses) || !SamePoints(c.points, start.points)) ++fail;
  }
  if (fail) {
    std::printf("%d checks failed\n", fail);
    return 1;
  }
  std::printf("SIM3 GRAPH FACADE TEST PASSED\n");
  return 0;
}
