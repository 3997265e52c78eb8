// GPU test of AddRelativePose on the C++ facades: relative-pose factors of a solver's own
// problem (ba_set_relative, any number of poses).  One stereo window of 9 poses (0 and 1
// fixed) carries an odometry chain over consecutive poses (its first factor ends on a fixed
// pose), a loop closure between two poses that share no landmark, one pair named twice in
// opposite orientations and one factor whose j is fixed.  Solve of FullBundleAdjustmentSolver
// and of FullBundleAdjustmentSolverRefactor with the factors in the caller's units must leave
// on their handles the poses and points that ba_set_relative + ba_solve give when called
// directly through include/ba_hip.h on the same arrays in scaled units (the facade's
// preprocessing restated here), bit for bit, and differ from a Solve without the factors.
// Exit code 0 = pass.
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
constexpr int kIters = 4, kPoses = 9, kPoints = 60, kWin = 3;

struct Window {
  std::vector<_BA_Camera> cams;
  std::vector<_BA_Pose> poses;
  std::vector<_BA_Point> points;
  std::vector<int> fixed_pose;
  struct Obs {
    int c, j, i;
    _BA_Pixel uv;
  };
  std::vector<Obs> obs;
};

// landmark i is seen by kWin consecutive poses only: the loop closure (8, 2) couples two poses
// that share no landmark
static Window MakeWindow(unsigned seed) {
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
  std::vector<_BA_Pose> truth(kPoses);
  for (int j = 0; j < kPoses; ++j) {
    truth[j] = _BA_Pose::Identity();
    truth[j].translation() = _BA_Point(0.25 * j, 0.02 * j * j, 0.03 * j);
  }
  std::vector<_BA_Point> Xt(kPoints);
  for (int i = 0; i < kPoints; ++i) Xt[i] = _BA_Point(0.5 + 1.6 * U(gen), 1.0 * U(gen), 6.0 + 2.5 * U(gen));
  for (int i = 0; i < kPoints; ++i) {
    const int j0 = i * (kPoses - kWin + 1) / kPoints;
    for (int j = j0; j < j0 + kWin; ++j)
      for (int c = 0; c < 2; ++c) {
        const _BA_Point Xc = w.cams[c].pose_this_to_cam0 * (truth[j].inverse() * Xt[i]);
        Window::Obs o;
        o.c = c;
        o.j = j;
        o.i = i;
        o.uv = _BA_Pixel(525.0 * Xc(0) / Xc(2) + 320.0, 525.0 * Xc(1) / Xc(2) + 240.0);
        w.obs.push_back(o);
      }
  }
  w.poses = truth;
  w.fixed_pose.assign(kPoses, 0);
  w.fixed_pose[0] = w.fixed_pose[1] = 1;
  for (int j = 2; j < kPoses; ++j) w.poses[j].translation() += _BA_Point(0.04 * U(gen), 0.04 * U(gen), 0.04 * U(gen));
  w.points = Xt;
  for (int i = 0; i < kPoints; ++i) w.points[i] += _BA_Point(0.15 * U(gen), 0.15 * U(gen), 0.15 * U(gen));
  return w;
}

static std::vector<Rel> MakeFactors(Window &w, double sigma) {
  std::vector<std::pair<int, int>> pairs;
  for (int q = 1; q + 1 < kPoses; ++q) pairs.emplace_back(q + 1, q);
  pairs.emplace_back(kPoses - 1, 2);
  pairs.emplace_back(3, 6);
  pairs.emplace_back(6, 3);
  pairs.emplace_back(0, 5);  // j fixed
  const double wgt = 1.0 / (sigma * sigma * 1e-4);
  std::vector<Rel> out;
  for (size_t f = 0; f < pairs.size(); ++f) {
    Rel r;
    r.pose_j = &w.poses[pairs[f].first];
    r.pose_k = &w.poses[pairs[f].second];
    r.measurement = r.pose_j->inverse() * (*r.pose_k);
    r.measurement.translation() += _BA_Point(0.01, -0.005 * (1.0 + f), 0.008);
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

#define TRY(expr)                                                          \
  do {                                                                     \
    if ((expr) != 0) {                                                     \
      std::printf("%s failed: %s\n", #expr, ba_last_error());              \
      return false;                                                        \
    }                                                                      \
  } while (0)

// the facade's preprocessing restated, then the C calls
static bool Direct(const Window &w, const std::vector<Rel> &rels, double sigma, const Options &options,
                   std::vector<double> *T, std::vector<double> *X, int64_t info[4]) {
  const double s = 0.01, inv = 100.0, wgt = 1.0 / (sigma * sigma * s * s);
  std::vector<double> intr, T_cj, Tp, Xp, uv, Z, Om;
  std::vector<uint8_t> pf, qf(w.points.size(), 0);
  std::vector<int32_t> oc, op, oq, rj, rk;
  for (const _BA_Camera &cam : w.cams) {
    intr.insert(intr.end(), {cam.fx * s, cam.fy * s, cam.cx * s, cam.cy * s});
    _BA_Pose P = cam.pose_this_to_cam0;
    P.translation() *= s;
    Pack(P, T_cj);
  }
  for (size_t j = 0; j < w.poses.size(); ++j) {
    _BA_Pose P = w.poses[j].inverse();
    P.translation() = P.translation() * s;
    Pack(P, Tp);
    pf.push_back(static_cast<uint8_t>(w.fixed_pose[j]));
  }
  for (const _BA_Point &Q : w.points) {
    const _BA_Point Qs = Q * s;
    for (int r = 0; r < 3; ++r) Xp.push_back(Qs(r));
  }
  for (const auto &o : w.obs) {
    oc.push_back(o.c);
    op.push_back(o.j);
    oq.push_back(o.i);
    uv.push_back(o.uv(0) * s);
    uv.push_back(o.uv(1) * s);
  }
  for (const Rel &r : rels) {
    rj.push_back(static_cast<int32_t>(r.pose_j - &w.poses[0]));
    rk.push_back(static_cast<int32_t>(r.pose_k - &w.poses[0]));
    _BA_Pose Zs = r.measurement;
    Zs.translation() = Zs.translation() * s;
    Pack(Zs, Z);
    for (int rr = 0; rr < 6; ++rr)
      for (int c = 0; c < 6; ++c)
        Om.push_back(((rr < 3 ? inv : 1.0) * r.information[6 * rr + c] * (c < 3 ? inv : 1.0)) / wgt);
  }
  ba_handle *h = nullptr;
  TRY(ba_create(&h, 0));
  TRY(ba_set_cameras(h, static_cast<int>(w.cams.size()), intr.data(), T_cj.data()));
  TRY(ba_set_poses(h, static_cast<int>(w.poses.size()), Tp.data(), pf.data()));
  TRY(ba_set_points(h, static_cast<int>(w.points.size()), Xp.data(), qf.data()));
  TRY(ba_set_observations(h, static_cast<int64_t>(oc.size()), oc.data(), op.data(), oq.data(), uv.data()));
  if (!rels.empty()) {
    TRY(ba_relative_check(static_cast<int>(w.poses.size()), pf.data(), static_cast<int64_t>(rj.size()), rj.data(),
                          rk.data(), Z.data(), Om.data()));
    TRY(ba_set_relative(h, static_cast<int64_t>(rj.size()), rj.data(), rk.data(), Z.data(), Om.data()));
  }
  TRY(ba_finalize(h));
  TRY(ba_relative_info(h, info));
  const ba_options o = MakeOptions(options);
  int n_iter = 0;
  TRY(ba_solve(h, &o, nullptr, 0, &n_iter, nullptr));
  T->resize(Tp.size());
  X->resize(Xp.size());
  TRY(ba_get_poses(h, T->data()));
  TRY(ba_get_points(h, X->data(), nullptr));
  ba_destroy(h);
  return n_iter == kIters;
}

static bool HandleState(ba_handle *h, size_t n_pose, size_t n_pt, std::vector<double> *T, std::vector<double> *X,
                        int64_t info[4]) {
  T->resize(12 * n_pose);
  X->resize(3 * n_pt);
  TRY(ba_get_poses(h, T->data()));
  TRY(ba_get_points(h, X->data(), nullptr));
  TRY(ba_relative_info(h, info));
  return true;
}

static bool Same(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}

int main() {
  const Window start = MakeWindow(1);
  const double sigma = 0.7;
  Options options;
  options.solver_type = SolverType::LEVENBERG_MARQUARDT;  // the refactored class selects by it
  options.iteration_handle.max_num_iterations = kIters;
  options.convergence_handle.threshold_step_size = 0.0;
  options.convergence_handle.threshold_cost_change = 0.0;
  int fail = 0;
  std::vector<double> T_rel, X_rel, T_free, X_free;
  int64_t info[4] = {0, 0, 0, 0}, info_free[4] = {0, 0, 0, 0};
  {
    Window w = start;
    const std::vector<Rel> rels = MakeFactors(w, sigma);
    if (!Direct(w, rels, sigma, options, &T_rel, &X_rel, info)) ++fail;
    if (!Direct(w, {}, sigma, options, &T_free, &X_free, info_free)) ++fail;
    std::printf("factors %lld coupled blocks %lld only-factor blocks %lld bytes %lld\n", (long long)info[0],
                (long long)info[1], (long long)info[2], (long long)info[3]);
    if (info[0] != static_cast<int64_t>(rels.size()) || info[2] < 1 || info_free[0] != 0) ++fail;
    if (Same(T_rel, T_free)) ++fail;  // the factors are felt
  }
  // ---- FullBundleAdjustmentSolver
  {
    Window w = start;
    const std::vector<Rel> rels = MakeFactors(w, sigma);
    FullBundleAdjustmentSolver s;
    s.SetVerbose(false);
    for (size_t c = 0; c < w.cams.size(); ++c) s.AddCamera(static_cast<int>(c), w.cams[c]);
    for (auto &T : w.poses) s.AddPose(&T);
    for (auto &X : w.points) s.AddPoint(&X);
    for (size_t j = 0; j < w.poses.size(); ++j)
      if (w.fixed_pose[j]) s.MakePoseFixed(&w.poses[j]);
    for (const auto &o : w.obs) s.AddObservation(o.c, &w.poses[o.j], &w.points[o.i], o.uv);
    for (const Rel &r : rels) s.AddRelativePose(r, sigma);
    _BA_Pose stranger = _BA_Pose::Identity();
    Rel bad = rels[0];
    bad.pose_k = &stranger;
    bool threw = false;
    try {
      s.AddRelativePose(bad, sigma);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    if (!threw) ++fail;
    if (!s.Solve(options)) ++fail;
    s.AddRelativePose(rels[0], sigma);  // finalized: warns, ignored
    std::vector<double> T, X;
    int64_t fi[4];
    if (!HandleState(s.GetHandle(), w.poses.size(), w.points.size(), &T, &X, fi)) ++fail;
    const bool same = Same(T, T_rel) && Same(X, X_rel);
    std::printf("FullBundleAdjustmentSolver: %s, factors %lld\n", same ? "same bits" : "DIFFERENT", (long long)fi[0]);
    if (!same || fi[0] != info[0] || fi[1] != info[1]) ++fail;
    // ReloadParameterValues keeps the factors, Reset drops them
    s.ReloadParameterValues();
    if (ba_relative_info(s.GetHandle(), fi) != 0 || fi[0] != info[0]) ++fail;
    s.Reset();
    if (s.GetHandle() != nullptr) ++fail;
  }
  // ---- FullBundleAdjustmentSolverRefactor
  {
    Window w = start;
    const std::vector<Rel> rels = MakeFactors(w, sigma);
    FullBundleAdjustmentSolverRefactor r;
    r.SetVerbose(false);
    for (size_t c = 0; c < w.cams.size(); ++c) {
      OptimizerCamera cam;
      cam.fx = w.cams[c].fx;
      cam.fy = w.cams[c].fy;
      cam.cx = w.cams[c].cx;
      cam.cy = w.cams[c].cy;
      cam.camera_to_body_pose = w.cams[c].pose_this_to_cam0;
      r.RegisterCamera(static_cast<int>(c), cam);
    }
    for (auto &T : w.poses) r.RegisterWorldToBodyPose(&T);
    for (auto &X : w.points) r.RegisterWorldPoint(&X);
    for (size_t j = 0; j < w.poses.size(); ++j)
      if (w.fixed_pose[j]) r.MakePoseFixed(&w.poses[j]);
    for (const auto &o : w.obs) r.AddObservation(o.c, &w.poses[o.j], &w.points[o.i], o.uv);
    for (const Rel &f : rels) r.AddRelativePose(f, sigma);
    if (!r.Solve(options)) ++fail;
    std::vector<double> T, X;
    int64_t fi[4];
    if (!HandleState(r.GetHandle(), w.poses.size(), w.points.size(), &T, &X, fi)) ++fail;
    const bool same = Same(T, T_rel) && Same(X, X_rel);
    std::printf("FullBundleAdjustmentSolverRefactor: %s, factors %lld\n", same ? "same bits" : "DIFFERENT", (long long)fi[0]);
    if (!same || fi[0] != info[0]) ++fail;
  }
  if (fail) {
    std::printf("%d checks failed\n", fail);
    return 1;
  }
  std::printf("RELATIVE FACADE TEST PASSED\n");
  return 0;
}
