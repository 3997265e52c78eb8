// GPU test of the robust kernels, covariance blocks and gate of the Sim(3) graph on the C++
// facades (RelativeSim3::robust_kind / robust_scale, SolveSim3Graph, GetRelativeSim3Weights,
// ComputeSim3GraphCovariance, GateSim3LoopClosures of FullBundleAdjustmentSolver and
// FullBundleAdjustmentSolverRefactor) on the loop scene of test_sim3_graph.cpp: 40 rigid keyframes
// on a circle whose map drifted in scale by c_q = exp(0.003 q).  Every facade call in the caller's
// units must give what ba_sim3_create + ba_sim3_set_robust + ba_sim3_solve / ba_sim3_factor_weights /
// ba_sim3_covariance / ba_sim3_gate give when called directly on the same arrays in scaled units
// (the facade's preprocessing restated here), bit for bit after the unit conversion.  robust_kind 0
// reproduces the plain solve, two values of sigma_pixel throw, and SolvePoseGraph (on the loop), Solve
// and SolveBatch (both classes, on a window of 12 keyframes with 40 landmarks) beside robust Sim(3)
// factors give the rows, poses and points they give without them, to the bit.  Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "ba_hip.h"
#include "core/full_bundle_adjustment_solver.h"
#include "core/full_bundle_adjustment_solver_refactor.h"
#include "eigen3/Eigen/Dense"

using namespace visual_navigation::analytic_solver;
using Sim = FullBundleAdjustmentSolver::RelativeSim3;
using Rel = FullBundleAdjustmentSolver::RelativePose;
using Mat7 = Eigen::Matrix<double, 7, 7>;
constexpr int kIters = 5, kPoses = 40;
constexpr double kSigma = 0.7, kScaler = 0.01, kInv = 100.0;

struct Scene {
  std::vector<_BA_Pose> poses, truth;
  std::vector<double> scale;
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
    _BA_Pose E = sc.truth[q].inverse() * sc.truth[q - 1];
    E.translation() = E.translation() * sc.scale[q];
    start_jw.push_back(E * start_jw.back());
  }
  for (const _BA_Pose &T : start_jw) sc.poses.push_back(T.inverse());
  return sc;
}

// the factors of the loop: the chain and three closures; robust: kinds 0, 1, 2, 3 in turn
static std::vector<Sim> MakeSim3(Scene &sc, bool robust) {
  const double wgt = 1.0 / (kSigma * kSigma * 1e-4);
  std::vector<std::pair<int, int>> pairs;
  for (int q = 1; q < kPoses; ++q) pairs.emplace_back(q, q - 1);
  pairs.emplace_back(kPoses - 1, 0);
  pairs.emplace_back(kPoses - 2, 1);
  pairs.emplace_back(2, kPoses - 3);
  std::vector<Sim> out;
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
    if (robust) {
      r.robust_kind = static_cast<int>(f % 4);
      r.robust_scale = 2.0 + static_cast<double>(f % 4);
    }
    out.push_back(r);
  }
  return out;
}

static ba_options MakeOptions(const Options &o) {
  ba_options c;
  c.threshold_step_size = o.convergence_handle.threshold_step_size;
  c.threshold_cost_change = o.convergence_handle.threshold_cost_change;
  c.threshold_huber_loss = o.outlier_handle.threshold_huber_loss;
  c.threshold_outlier_rejection = o.outlier_handle.threshold_outlier_rejection;
  c.max_num_iterations = o.iteration_handle.max_num_iterations;
  c.initial_lambda = o.trust_region_handle.initial_lambda;
  c.decrease_ratio_lambda = o.trust_region_handle.decrease_ratio_lambda;
  c.increase_ratio_lambda = o.trust_region_handle.increase_ratio_lambda;
  c.gauss_newton = 0;
  return c;
}

#define TRY(expr)                                             \
  do {                                                        \
    if ((expr) != 0) {                                        \
      std::printf("%s failed: %s\n", #expr, ba_last_error()); \
      return false;                                           \
    }                                                         \
  } while (0)

// the facade's preprocessing restated: poses as similarities, one factor or candidate
struct Arrays {
  std::vector<double> S, Z, Om, scale;
  std::vector<uint8_t> pf;
  std::vector<int32_t> j, k, kind;
};
static void PackOne(const Scene &sc, const Sim &r, std::vector<int32_t> *j, std::vector<int32_t> *k,
                    std::vector<double> *Z, std::vector<double> *Om) {
  const double wgt = 1.0 / (kSigma * kSigma * kScaler * kScaler);
  j->push_back(static_cast<int32_t>(r.pose_j - &sc.poses[0]));
  k->push_back(static_cast<int32_t>(r.pose_k - &sc.poses[0]));
  const double *M = r.measurement;
  const double det = M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) +
                     M[2] * (M[4] * M[9] - M[5] * M[8]);
  const double sz = std::cbrt(det);
  for (int a = 0; a < 3; ++a)
    for (int c = 0; c < 3; ++c) Z->push_back(M[4 * a + c] / sz);
  for (int a = 0; a < 3; ++a) Z->push_back(M[4 * a + 3] * kScaler);
  Z->push_back(sz);
  for (int a = 0; a < 7; ++a)
    for (int c = 0; c < 7; ++c) Om->push_back(((a < 3 ? kInv : 1.0) * r.information[7 * a + c] * (c < 3 ? kInv : 1.0)) / wgt);
}
static Arrays Pack(const Scene &sc, const std::vector<Sim> &rels) {
  Arrays a;
  a.pf.assign(sc.poses.size(), 0);
  a.pf[0] = 1;
  for (const _BA_Pose &pose : sc.poses) {
    _BA_Pose P = pose.inverse();
    P.translation() = P.translation() * kScaler;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) a.S.push_back(P.linear()(r, c));
    for (int r = 0; r < 3; ++r) a.S.push_back(P.translation()(r));
    a.S.push_back(1.0);
  }
  for (const Sim &r : rels) {
    PackOne(sc, r, &a.j, &a.k, &a.Z, &a.Om);
    a.kind.push_back(r.robust_kind);
    a.scale.push_back(r.robust_kind ? r.robust_scale * (kSigma * kScaler) : 0.0);  // times the unit, as the facade
  }
  return a;
}

struct Direct {
  std::vector<double> S_new, s, w, cov_pose, cov_cross, cov_rel, d2;
  std::vector<ba_iter_info> rows;
};

// sel / pairs / cands: registration indices; the covariance and the gate at the START poses, then the solve
static bool RunDirect(const Scene &sc, const std::vector<Sim> &rels, const Options &options,
                      const std::vector<int32_t> &sel, const std::vector<int32_t> &pj, const std::vector<int32_t> &pk,
                      const std::vector<Sim> &cands, Direct *out) {
  const Arrays a = Pack(sc, rels);
  const int n = static_cast<int>(sc.poses.size());
  const int64_t F = static_cast<int64_t>(a.j.size());
  ba_handle *h = nullptr;
  TRY(ba_create(&h, 0));
  ba_sim3 *g = nullptr;
  TRY(ba_sim3_create(&g, h, n, a.S.data(), a.pf.data(), F, a.j.data(), a.k.data(), a.Z.data(), a.Om.data()));
  TRY(ba_sim3_set_robust(g, a.kind.data(), a.scale.data()));
  out->cov_pose.assign(49 * sel.size(), 0.0);
  out->cov_cross.assign(49 * pj.size(), 0.0);
  out->cov_rel.assign(49 * pj.size(), 0.0);
  int64_t dropped = -1;
  if (!sel.empty() || !pj.empty()) {
    TRY(ba_sim3_covariance(g, static_cast<int>(sel.size()), sel.data(), out->cov_pose.data(),
                           static_cast<int64_t>(pj.size()), pj.data(), pk.data(), out->cov_cross.data(),
                           out->cov_rel.data(), &dropped));
    if (dropped != 0) return false;
  }
  if (!cands.empty()) {
    std::vector<int32_t> cj, ck;
    std::vector<double> Z, Om;
    for (const Sim &c : cands) PackOne(sc, c, &cj, &ck, &Z, &Om);
    out->d2.assign(cands.size(), 0.0);
    TRY(ba_sim3_gate(g, static_cast<int64_t>(cands.size()), cj.data(), ck.data(), Z.data(), Om.data(), out->d2.data(),
                     nullptr, nullptr, &dropped));
    if (dropped != 0) return false;
  }
  const ba_options o = MakeOptions(options);
  out->rows.assign(kIters, ba_iter_info());
  int n_iter = 0, converged = 0;
  TRY(ba_sim3_solve(g, &o, out->rows.data(), kIters, &n_iter, &converged));
  out->S_new.assign(a.S.size(), 0.0);
  TRY(ba_sim3_get_poses(g, out->S_new.data()));
  out->s.assign(static_cast<size_t>(F), 0.0);
  out->w.assign(static_cast<size_t>(F), 0.0);
  TRY(ba_sim3_factor_weights(g, out->s.data(), out->w.data()));
  ba_sim3_destroy(g);
  ba_destroy(h);
  return n_iter == kIters;
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

// the written-back poses are the direct call's: T_jw = [R, t / s] in the caller's units, inverted
static bool SamePoses(const Scene &sc, const std::vector<_BA_Pose> &got, const std::vector<double> &Sn) {
  for (size_t p = 1; p < got.size(); ++p) {
    _BA_Pose T_jw;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) T_jw.linear()(r, c) = Sn[13 * p + 3 * r + c];
      T_jw.translation()(r) = Sn[13 * p + 9 + r] / Sn[13 * p + 12];
    }
    T_jw.translation() *= kInv;
    const _BA_Pose want = T_jw.inverse();
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c)
        if (got[p].linear()(r, c) != want.linear()(r, c)) return false;
      if (got[p].translation()(r) != want.translation()(r)) return false;
    }
  }
  return true;
}

static bool SameBlocks(const std::vector<Mat7> &got, const std::vector<double> &scaled) {
  const double unit = kSigma * kScaler;
  if (got.size() * 49 != scaled.size()) return false;
  for (size_t b = 0; b < got.size(); ++b)
    for (int r = 0; r < 7; ++r)
      for (int c = 0; c < 7; ++c) {
        const double want = (unit * unit) * ((r < 3 ? kInv : 1.0) * scaled[49 * b + 7 * r + c] * (c < 3 ? kInv : 1.0));
        if (got[b](r, c) != want) return false;
      }
  return true;
}

static bool IsZero(const Mat7 &m) {
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c)
      if (m(r, c) != 0.0) return false;
  return true;
}

template <class Solver>
static int Check(const char *name, const Scene &start, const Options &options) {
  int fail = 0;
  const std::vector<int32_t> sel = {39, 7, 22, 7}, pj = {39, 1, 0, 12, 5}, pk = {1, 39, 7, 0, 6};
  for (int robust = 0; robust < 2; ++robust) {
    Scene sc = start, dc = start;
    const std::vector<Sim> rels = MakeSim3(sc, robust != 0), drels = MakeSim3(dc, robust != 0);
    std::vector<Sim> cands(rels.end() - 3, rels.end()), dcands(drels.end() - 3, drels.end());
    cands.push_back(cands.back());
    dcands.push_back(dcands.back());
    for (int e = 0; e < 3; ++e)
      for (int c = 0; c < 3; ++c) {  // the last closure again with 1.3 times the scale
        cands.back().measurement[4 * e + c] *= 1.3;
        dcands.back().measurement[4 * e + c] *= 1.3;
      }
    Direct want;
    if (!RunDirect(dc, drels, options, sel, pj, pk, dcands, &want)) return 1;
    Solver s;
    s.SetVerbose(false);
    for (auto &T : sc.poses) {
      if constexpr (std::is_same<Solver, FullBundleAdjustmentSolver>::value)
        s.AddPose(&T);
      else
        s.RegisterWorldToBodyPose(&T);
    }
    s.MakePoseFixed(&sc.poses[0]);
    for (const Sim &r : rels) s.AddRelativeSim3(r, kSigma);
    bool threw = false;
    try {
      s.GetRelativeSim3Weights(nullptr, nullptr);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    if (!threw) ++fail;
    std::vector<_BA_Pose *> poses;
    std::vector<std::pair<_BA_Pose *, _BA_Pose *>> pairs;
    for (int32_t p : sel) poses.push_back(&sc.poses[p]);
    for (size_t p = 0; p < pj.size(); ++p) pairs.emplace_back(&sc.poses[pj[p]], &sc.poses[pk[p]]);
    std::vector<Mat7> cp, cc, cr;
    if (!s.ComputeSim3GraphCovariance(poses, pairs, &cp, &cc, &cr)) ++fail;
    const bool cov = SameBlocks(cp, want.cov_pose) && SameBlocks(cc, want.cov_cross) && SameBlocks(cr, want.cov_rel) &&
                     cp[1] == cp[3] && IsZero(cc[2]) && IsZero(cc[3]) && !IsZero(cc[0]);
    std::vector<double> d2;
    if (!s.GateSim3LoopClosures(cands, kSigma, &d2)) ++fail;
    const double unit = kSigma * kScaler;
    bool gate = d2.size() == want.d2.size();
    for (size_t c = 0; gate && c < d2.size(); ++c) gate = d2[c] == want.d2[c] / (unit * unit);
    Summary summary;
    std::vector<double> scales, gs, gw;
    if (!s.SolveSim3Graph(options, &summary, nullptr, &scales)) ++fail;
    s.GetRelativeSim3Weights(&gs, &gw);
    bool solve = SameRows(summary, want.rows) && SamePoses(sc, sc.poses, want.S_new) && gs.size() == want.s.size();
    bool bites = false;
    for (size_t f = 0; solve && f < gs.size(); ++f) {
      solve = gs[f] == want.s[f] / (unit * unit) && gw[f] == want.w[f] && scales[f < scales.size() ? f : 0] > 0.0;
      if (rels[f].robust_kind == 0 && gw[f] != 1.0) solve = false;
      bites = bites || gw[f] < 1.0;
    }
    std::printf("%s, robust %d: covariance %s, gate %s (d2 %.3g %.3g %.3g | %.3g), solve and weights %s\n", name, robust,
                cov ? "same bits" : "DIFFERENT", gate ? "same bits" : "DIFFERENT", d2[0], d2[1], d2[2], d2[3],
                solve ? "same bits" : "DIFFERENT");
    if (!cov || !gate || !solve || (robust == 0 && bites)) ++fail;
  }
  return fail;
}

// ---- Solve and SolveBatch beside robust Sim(3) factors: a window of 12 keyframes (two fixed) that
// ---- see 40 landmarks through one camera, solved with and without the factors registered
struct Window {
  std::vector<_BA_Pose> poses;
  std::vector<_BA_Point> points;
  std::vector<_BA_Pixel> uv;  // pose-major: uv[j * points + i]
};
static Window MakeWindow() {
  Window w;
  std::vector<_BA_Pose> truth(12);
  for (int j = 0; j < 12; ++j) {
    truth[j] = _BA_Pose::Identity();
    truth[j].translation() = _BA_Point(0.25 * j, 0.02 * j * j, 0.03 * j);
  }
  for (int i = 0; i < 40; ++i) {
    const double a = 0.37 * i, b = 0.91 * i;
    w.points.push_back(_BA_Point(0.5 + 1.6 * std::sin(a), std::cos(b), 6.0 + 2.5 * std::sin(a + b)));
  }
  for (int j = 0; j < 12; ++j)
    for (int i = 0; i < 40; ++i) {
      const _BA_Point Xc = truth[j].inverse() * w.points[i];
      w.uv.push_back(_BA_Pixel(525.0 * Xc(0) / Xc(2) + 320.0, 525.0 * Xc(1) / Xc(2) + 240.0));
    }
  w.poses = truth;
  for (int j = 2; j < 12; ++j) w.poses[j].translation() += _BA_Point(0.03 * std::sin(1.3 * j), 0.02 * std::cos(2.1 * j), 0.025);
  for (int i = 0; i < 40; ++i) w.points[i] += _BA_Point(0.1 * std::sin(0.7 * i), 0.1 * std::cos(1.9 * i), 0.12 * std::sin(2.3 * i));
  return w;
}

template <class Solver>
static void RegisterWindow(Solver &s, Window &w, bool sim3) {
  s.SetVerbose(false);
  if constexpr (std::is_same<Solver, FullBundleAdjustmentSolver>::value) {
    _BA_Camera cam;
    cam.fx = cam.fy = 525.0;
    cam.cx = 320.0;
    cam.cy = 240.0;
    cam.pose_this_to_cam0 = _BA_Pose::Identity();
    s.AddCamera(0, cam);
    for (auto &T : w.poses) s.AddPose(&T);
    for (auto &X : w.points) s.AddPoint(&X);
  } else {
    OptimizerCamera cam;
    cam.fx = cam.fy = 525.0;
    cam.cx = 320.0;
    cam.cy = 240.0;
    cam.camera_to_body_pose = _BA_Pose::Identity();
    s.RegisterCamera(0, cam);
    for (auto &T : w.poses) s.RegisterWorldToBodyPose(&T);
    for (auto &X : w.points) s.RegisterWorldPoint(&X);
  }
  s.MakePoseFixed(&w.poses[0]);
  s.MakePoseFixed(&w.poses[1]);
  for (size_t j = 0; j < w.poses.size(); ++j)
    for (size_t i = 0; i < w.points.size(); ++i) s.AddObservation(0, &w.poses[j], &w.points[i], w.uv[j * w.points.size() + i]);
  for (size_t j = 1; sim3 && j < w.poses.size(); ++j) {  // robust Sim(3) factors that no BA path may see
    Sim r;
    r.pose_j = &w.poses[j];
    r.pose_k = &w.poses[j - 1];
    r.measurement[3] = 0.3;
    r.measurement[0] = r.measurement[5] = r.measurement[10] = 1.1;
    for (int a = 0; a < 7; ++a) r.information[8 * a] = 50.0;
    r.robust_kind = 1 + static_cast<int>(j % 3);
    r.robust_scale = 0.5;
    s.AddRelativeSim3(r, kSigma);
  }
}

static bool SameWindow(const Window &a, const Window &b, const Summary &sa, const Summary &sb) {
  bool same = a.poses.size() == b.poses.size() && a.points.size() == b.points.size();
  for (size_t j = 0; same && j < a.poses.size(); ++j) same = a.poses[j].matrix() == b.poses[j].matrix();
  for (size_t i = 0; same && i < a.points.size(); ++i) same = a.points[i] == b.points[i];
  const auto &ra = sa.GetOptimizationInfoList(), &rb = sb.GetOptimizationInfoList();
  same = same && !ra.empty() && ra.size() == rb.size();
  for (size_t k = 0; same && k < ra.size(); ++k)
    same = ra[k].cost == rb[k].cost && ra[k].damping_term == rb[k].damping_term && ra[k].abs_step == rb[k].abs_step &&
           ra[k].iteration_status == rb[k].iteration_status;
  return same;
}

template <class Solver>
static int CheckBa(const char *name, const Options &options) {
  const Window start = MakeWindow();
  int fail = 0;
  for (int batch = 0; batch < 2; ++batch) {
    Window a = start, b = start;
    Solver with, without;
    RegisterWindow(with, a, true);
    RegisterWindow(without, b, false);
    Summary sa, sb;
    bool ok;
    if (batch) {
      std::vector<Summary> va(1), vb(1);
      ok = Solver::SolveBatch({&with}, options, &va, nullptr, kSigma) && Solver::SolveBatch({&without}, options, &vb, nullptr, kSigma);
      sa = va[0];
      sb = vb[0];
    } else {
      ok = with.Solve(options, &sa) && without.Solve(options, &sb);
    }
    bool moved = false;
    for (size_t j = 0; j < a.poses.size(); ++j) moved = moved || !(a.poses[j].matrix() == start.poses[j].matrix());
    const bool same = ok && moved && SameWindow(a, b, sa, sb);
    std::printf("%s, %s beside robust Sim(3) factors: %s\n", name, batch ? "SolveBatch" : "Solve", same ? "same bits" : "DIFFERENT");
    if (!same) ++fail;
  }
  return fail;
}

int main() {
  const Scene start = MakeScene();
  Options options;
  options.solver_type = SolverType::LEVENBERG_MARQUARDT;
  options.iteration_handle.max_num_iterations = kIters;
  options.convergence_handle.threshold_step_size = -1.0;
  options.convergence_handle.threshold_cost_change = -1.0;
  options.trust_region_handle.initial_lambda = 1e-4;
  int fail = 0;
  fail += Check<FullBundleAdjustmentSolver>("FullBundleAdjustmentSolver", start, options);
  fail += Check<FullBundleAdjustmentSolverRefactor>("FullBundleAdjustmentSolverRefactor", start, options);
  // ---- the robust solve differs from the plain one; robust_kind 0 is the plain one
  {
    Scene a = start, b = start;
    const std::vector<Sim> ra = MakeSim3(a, true), rb = MakeSim3(b, false);
    Direct da, db;
    if (!RunDirect(a, ra, options, {}, {}, {}, {}, &da) || !RunDirect(b, rb, options, {}, {}, {}, {}, &db)) ++fail;
    if (da.rows[0].trial_cost == db.rows[0].trial_cost) ++fail;
  }
  // ---- two values of sigma_pixel throw; a refused kernel throws when the factor is added
  {
    Scene sc = start;
    std::vector<Sim> rels = MakeSim3(sc, true);
    FullBundleAdjustmentSolver s;
    s.SetVerbose(false);
    for (auto &T : sc.poses) s.AddPose(&T);
    s.MakePoseFixed(&sc.poses[0]);
    for (const Sim &r : rels) s.AddRelativeSim3(r, kSigma);
    std::vector<double> d2;
    int threw = 0;
    try {
      s.GateSim3LoopClosures({rels.back()}, 1.0, &d2);
    } catch (const std::runtime_error &e) {
      threw += std::string(e.what()).find("sigma_pixel = 0.7 and 1") != std::string::npos;
    }
    Sim bad = rels[0];
    bad.robust_kind = 2;
    bad.robust_scale = 0.0;
    try {
      s.AddRelativeSim3(bad, kSigma);
    } catch (const std::runtime_error &e) {
      threw += std::string(e.what()).find("scale must be > 0") != std::string::npos;
    }
    s.AddRelativeSim3(rels[0], 0.5);
    std::vector<Mat7> cp;
    try {
      s.ComputeSim3GraphCovariance({&sc.poses[3]}, {}, &cp, nullptr, nullptr);
    } catch (const std::runtime_error &e) {
      threw += std::string(e.what()).find("sigma_pixel = 0.7 and 0.5") != std::string::npos;
    }
    std::printf("refusals: %d of 3\n", threw);
    if (threw != 3) ++fail;
  }
  // ---- SolvePoseGraph beside robust Sim(3) factors ignores them
  {
    Scene a = start, b = start;
    const std::vector<Sim> sim_a = MakeSim3(a, true);
    FullBundleAdjustmentSolver both, only;
    both.SetVerbose(false);
    only.SetVerbose(false);
    for (auto &T : a.poses) both.AddPose(&T);
    for (auto &T : b.poses) only.AddPose(&T);
    both.MakePoseFixed(&a.poses[0]);
    only.MakePoseFixed(&b.poses[0]);
    for (const Sim &f : sim_a) both.AddRelativeSim3(f, kSigma);
    const double wgt = 1.0 / (kSigma * kSigma * 1e-4);
    for (Scene *sc : {&a, &b})
      for (int q = 1; q < kPoses; ++q) {
        Rel r;
        r.pose_j = &sc->poses[q];
        r.pose_k = &sc->poses[q - 1];
        r.measurement = sc->poses[q].inverse() * sc->poses[q - 1];
        r.measurement.translation() += _BA_Point(0.01, -0.005, 0.008);
        for (int e = 0; e < 6; ++e) r.information[6 * e + e] = wgt * (e < 3 ? 2.0 : 2e2);
        (sc == &a ? both : only).AddRelativePose(r, kSigma);
      }
    if (!both.SolvePoseGraph(options) || !only.SolvePoseGraph(options)) ++fail;
    bool same = true, moved = false;
    for (int p = 0; p < kPoses; ++p) {
      same = same && a.poses[p].matrix() == b.poses[p].matrix();
      moved = moved || !(a.poses[p].matrix() == start.poses[p].matrix());
    }
    std::printf("SolvePoseGraph beside robust Sim(3) factors: %s\n", same && moved ? "same bits" : "DIFFERENT");
    if (!same || !moved) ++fail;
  }
  fail += CheckBa<FullBundleAdjustmentSolver>("FullBundleAdjustmentSolver", options);
  fail += CheckBa<FullBundleAdjustmentSolverRefactor>("FullBundleAdjustmentSolverRefactor", options);
  if (fail) {
    std::printf("%d checks failed\n", fail);
    return 1;
  }
  std::printf("SIM3 ROBUST COV FACADE TEST PASSED\n");
  return 0;
}
