// GPU test of robust loop-closure factors on the C++ facades (RelativePose::robust_kind /
// robust_scale, SolvePoseGraph, GetRelativeWeights; ba_pgraph_set_robust and
// ba_pgraph_factor_report of include/ba_hip.h).  A chain of 12 poses (pose 0 fixed) with drifted
// start values carries an odometry chain and four loop closures, one of them false (its
// measurement is 2 units off).  The closures carry a Cauchy kernel with a Mahalanobis scale given
// in the caller's units.  SolvePoseGraph of FullBundleAdjustmentSolver and of
// FullBundleAdjustmentSolverRefactor must leave behind the caller's pointers the poses that
// ba_pgraph_create + ba_pgraph_set_robust + ba_pgraph_solve give when called directly on the same
// arrays in scaled units (the facade's preprocessing restated here, the scale times sigma_pixel *
// 0.01), bit for bit, with the same rows; GetRelativeWeights returns the weights of
// ba_pgraph_factor_report to the bit and s in the caller's units; the false closure ends with a
// small weight and the true ones near 1; without the kernel the result differs.  Then the
// refusals: a kind outside 0..3 and a scale <= 0 at AddRelativePose; FinalizeParameters, Solve and
// SolveBatch on a factor that carries a kernel ("pose-graph only").
// Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "ba_hip.h"
#include "core/full_bundle_adjustment_solver.h"
#include "core/full_bundle_adjustment_solver_refactor.h"
#include "eigen3/Eigen/Dense"

using namespace visual_navigation::analytic_solver;
using Rel = FullBundleAdjustmentSolver::RelativePose;
constexpr int kIters = 8, kPoses = 12, kChain = kPoses - 1, kFalse = kChain + 3;
constexpr double kScale = 3.0;  // Mahalanobis distance, caller's units

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

// robust: the closures carry the kernel `kind`
static std::vector<Rel> MakeFactors(Graph &g, double sigma, int kind) {
  std::vector<std::pair<int, int>> pairs;
  for (int q = 0; q + 1 < kPoses; ++q) pairs.emplace_back(q + 1, q);
  pairs.emplace_back(kPoses - 1, 2);
  pairs.emplace_back(3, 9);
  pairs.emplace_back(0, 6);  // j fixed
  pairs.emplace_back(10, 4);  // the false closure (index kFalse)
  const double wgt = 1.0 / (sigma * sigma * 1e-4);
  std::vector<Rel> out;
  for (size_t f = 0; f < pairs.size(); ++f) {
    Rel r;
    r.pose_j = &g.poses[pairs[f].first];
    r.pose_k = &g.poses[pairs[f].second];
    r.measurement = g.truth[pairs[f].first].inverse() * g.truth[pairs[f].second];
    r.measurement.translation() += _BA_Point(0.001, -0.0005 * (1.0 + f), 0.0008);
    if (static_cast<int>(f) == kFalse) r.measurement.translation() += _BA_Point(2.0, -1.0, 0.5);
    for (int a = 0; a < 6; ++a) {
      const double da = a < 3 ? 0.01 : 1.0;
      r.information[6 * a + a] = wgt * da * (a < 3 ? 2e4 : 2e2) * da;
    }
    r.information[6 * 4 + 1] = r.information[6 * 1 + 4] = wgt * 0.01 * 3e2;
    if (static_cast<int>(f) >= kChain) {
      r.robust_kind = kind;
      r.robust_scale = kind ? kScale : 0.0;
    }
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

struct DirectResult {
  std::vector<_BA_Pose> poses;  // as the write-back converts them
  std::vector<ba_iter_info> rows;
  std::vector<double> s, w;     // the factor report: s in the caller's units
};

// the facade's preprocessing restated, then the C calls
static bool Direct(const Graph &g, const std::vector<Rel> &rels, double sigma, const Options &options,
                   DirectResult *out) {
  const double s = 0.01, inv = 100.0, wgt = 1.0 / (sigma * sigma * s * s), unit = sigma * s;
  std::vector<double> Tp, Z, Om, scale;
  std::vector<uint8_t> pf(g.poses.size(), 0);
  pf[0] = 1;
  std::vector<int32_t> rj, rk, kind;
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
    kind.push_back(r.robust_kind);
    scale.push_back(r.robust_kind ? r.robust_scale * unit : 0.0);
  }
  const int64_t F = static_cast<int64_t>(rj.size());
  TRY(ba_pgraph_robust_check(F, kind.data(), scale.data()));
  ba_handle *h = nullptr;
  TRY(ba_create(&h, 0));
  ba_pgraph *pg = nullptr;
  TRY(ba_pgraph_create(&pg, h, static_cast<int>(g.poses.size()), Tp.data(), pf.data(), F, rj.data(), rk.data(),
                       Z.data(), Om.data()));
  TRY(ba_pgraph_set_robust(pg, kind.data(), scale.data()));
  const ba_options o = MakeOptions(options, false);
  out->rows.assign(kIters, ba_iter_info());
  int n_iter = 0, converged = 0;
  TRY(ba_pgraph_solve(pg, &o, out->rows.data(), kIters, &n_iter, &converged));
  std::vector<double> T(Tp.size());
  TRY(ba_pgraph_get_poses(pg, T.data()));
  out->s.assign(F, 0.0);
  out->w.assign(F, 0.0);
  TRY(ba_pgraph_factor_report(pg, out->s.data(), out->w.data()));
  for (double &v : out->s) v /= unit * unit;
  ba_pgraph_destroy(pg);
  ba_destroy(h);
  out->poses.clear();
  for (size_t p = 0; p < g.poses.size(); ++p) {
    _BA_Pose T_jw;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T_jw.linear()(r, c) = T[12 * p + 3 * r + c];
      T_jw.translation()(r) = T[12 * p + 9 + r];
    }
    T_jw.translation() *= static_cast<float>(inv);
    out->poses.push_back(p == 0 ? g.poses[0] : T_jw.inverse());
  }
  return n_iter == kIters;
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

static double Distance(const std::vector<_BA_Pose> &a, const std::vector<_BA_Pose> &b) {
  double d = 0.0;
  for (size_t p = 0; p < a.size(); ++p) d = std::max(d, (a[p].translation() - b[p].translation()).norm());
  return d;
}

template <class F>
static bool Throws(F &&f, const char *needle) {
  try {
    f();
  } catch (const std::runtime_error &e) {
    const bool ok = std::string(e.what()).find(needle) != std::string::npos;
    if (!ok) std::printf("threw \"%s\", expected \"%s\"\n", e.what(), needle);
    return ok;
  }
  std::printf("did not throw (expected \"%s\")\n", needle);
  return false;
}

template <class Solver>
static int FacadeCase(const char *name, const Graph &start, double sigma, const Options &options,
                      const DirectResult &want, void (*add_pose)(Solver &, _BA_Pose *)) {
  int fail = 0;
  Graph g = start;
  const std::vector<Rel> rels = MakeFactors(g, sigma, 2);
  Solver s;
  s.SetVerbose(false);
  for (auto &T : g.poses) add_pose(s, &T);
  s.MakePoseFixed(&g.poses[0]);
  for (const Rel &r : rels) s.AddRelativePose(r, sigma);
  if (!Throws([&] { s.GetRelativeWeights(nullptr, nullptr); }, "SolvePoseGraph has not run")) ++fail;
  Summary summary;
  if (!s.SolvePoseGraph(options, &summary)) ++fail;
  std::vector<double> fs, fw;
  s.GetRelativeWeights(&fs, &fw);
  const bool same = SamePoses(g.poses, want.poses) && SameRows(summary, want.rows) && fw == want.w && fs == want.s;
  std::printf("%s: %s\n", name, same ? "same bits" : "DIFFERENT");
  if (!same) ++fail;
  // the BA paths refuse the factors that carry a kernel
  if (!Throws([&] { s.Solve(options); }, "FinalizeParameters: factor 11 carries a robust kernel; robust factors are "
                                         "pose-graph only"))
    ++fail;
  Rel bad = rels[kFalse];
  bad.robust_kind = 4;
  if (!Throws([&] { s.AddRelativePose(bad, sigma); }, "kind = 4 is not one of 0..3")) ++fail;
  bad.robust_kind = 3;
  bad.robust_scale = 0.0;
  if (!Throws([&] { s.AddRelativePose(bad, sigma); }, "scale must be > 0")) ++fail;
  return fail;
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
  DirectResult robust, plain, clean;
  {
    Graph g = start;
    if (!Direct(g, MakeFactors(g, sigma, 2), sigma, options, &robust)) ++fail;
    if (!Direct(g, MakeFactors(g, sigma, 0), sigma, options, &plain)) ++fail;
    std::vector<Rel> without = MakeFactors(g, sigma, 0);
    without.erase(without.begin() + kFalse);
    if (!Direct(g, without, sigma, options, &clean)) ++fail;
    if (fail) {
      std::printf("the direct calls failed\n");
      return 1;
    }
    const double d_plain = Distance(plain.poses, clean.poses), d_robust = Distance(robust.poses, clean.poses);
    double w_in = 1.0;
    for (int f = kChain; f < kFalse; ++f) w_in = std::min(w_in, robust.w[f]);
    std::printf("distance to the solve without the false closure: no kernel %.4f, Cauchy %.4f; weight of the false "
                "closure %.3e (s = %.3e), smallest weight of a true closure %.3f\n",
                d_plain, d_robust, robust.w[kFalse], robust.s[kFalse], w_in);
    if (!(d_plain > 0.05) || !(d_robust < 0.2 * d_plain)) ++fail;
    if (!(robust.w[kFalse] < 1e-2) || !(w_in > 0.8)) ++fail;
    for (int f = 0; f < kChain; ++f)
      if (robust.w[f] != 1.0) ++fail;  // no kernel on the chain
    for (double w : plain.w)
      if (w != 1.0) ++fail;
    // w is the Cauchy weight of s in the caller's units with the caller's scale
    for (size_t f = kChain; f < robust.w.size(); ++f)
      if (std::fabs(robust.w[f] - 1.0 / (1.0 + robust.s[f] / (kScale * kScale))) > 1e-9 * robust.w[f]) ++fail;
  }
  fail += FacadeCase<FullBundleAdjustmentSolver>(
      "FullBundleAdjustmentSolver", start, sigma, options, robust,
      [](FullBundleAdjustmentSolver &s, _BA_Pose *T) { s.AddPose(T); });
  fail += FacadeCase<FullBundleAdjustmentSolverRefactor>(
      "FullBundleAdjustmentSolverRefactor", start, sigma, options, robust,
      [](FullBundleAdjustmentSolverRefactor &s, _BA_Pose *T) { s.RegisterWorldToBodyPose(T); });
  // ---- SolveBatch takes no factor that carries a kernel (a camera and a point are registered
  // so that the factors are looked at; the refusal comes before anything reaches the GPU)
  {
    Graph g = start;
    _BA_Camera cam;
    cam.fx = cam.fy = 525.0;
    cam.cx = 320.0;
    cam.cy = 240.0;
    cam.pose_this_to_cam0 = _BA_Pose::Identity();
    _BA_Point X(1.0, 1.0, 6.0);
    FullBundleAdjustmentSolver s;
    s.SetVerbose(false);
    s.AddCamera(0, cam);
    for (auto &T : g.poses) s.AddPose(&T);
    s.AddPoint(&X);
    s.MakePoseFixed(&g.poses[0]);
    const std::vector<std::vector<Rel>> lists(1, MakeFactors(g, sigma, 1));
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch({&s}, options, nullptr, nullptr, sigma, &lists); },
                "pose-graph only"))
      ++fail;
  }
  if (fail) {
    std::printf("%d checks failed\n", fail);
    return 1;
  }
  std::printf("POSE GRAPH ROBUST FACADE TEST PASSED\n");
  return 0;
}
