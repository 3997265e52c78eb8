// GPU test of FullBundleAdjustmentSolver::ComputeCovariance on the one-tile scene (mono,
// 3 poses with 1 fixed = 12 columns of the reduced system, 12 free landmarks and 2 fixed
// ones, which take the scale gauge out): the facade's blocks must equal ba_covariance on
// the facade's own handle after the unit conversion (Cov_pose = sigma^2 1e-4 D Sigma_s D,
// D = diag(100 I3, I3); Cov_point = sigma^2 Sigma_s) to 1e-14 relative — the same
// arithmetic, only the scaling differs —, before and after a Solve; an unregistered or
// fixed pointer throws; the refactored class forwards the call.  Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <random>
#include <stdexcept>
#include <vector>

#include "ba_hip.h"
#include "core/full_bundle_adjustment_solver.h"
#include "core/full_bundle_adjustment_solver_refactor.h"
#include "eigen3/Eigen/Dense"

using namespace visual_navigation::analytic_solver;

struct Scene {
  _BA_Camera cam;
  std::vector<_BA_Pose> poses;
  std::vector<_BA_Point> points;
  struct Obs {
    int j, i;
    _BA_Pixel uv;
  };
  std::vector<Obs> obs;
};

static Scene MakeScene() {
  std::mt19937 gen(5);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  Scene w;
  w.cam.fx = w.cam.fy = 525.0;
  w.cam.cx = 320.0;
  w.cam.cy = 240.0;
  w.cam.pose_this_to_cam0 = _BA_Pose::Identity();
  std::vector<_BA_Pose> truth(3);
  for (int j = 0; j < 3; ++j) {
    truth[j] = _BA_Pose::Identity();
    truth[j].translation() = _BA_Point(0.3 * j, 0.05 * j * j, 0.04 * j);
  }
  std::vector<_BA_Point> Xt(14);
  for (int i = 0; i < 14; ++i) Xt[i] = _BA_Point(0.4 + 1.5 * U(gen), 1.0 * U(gen), 6.0 + 2.5 * U(gen));
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 14; ++i) {
      const _BA_Point Xc = truth[j].inverse() * Xt[i];
      w.obs.push_back({j, i, _BA_Pixel(525.0 * Xc(0) / Xc(2) + 320.0, 525.0 * Xc(1) / Xc(2) + 240.0)});
    }
  w.poses = truth;
  for (int j = 1; j < 3; ++j) w.poses[j].translation() += _BA_Point(0.03 * U(gen), 0.03 * U(gen), 0.03 * U(gen));
  w.points = Xt;
  for (int i = 0; i < 12; ++i) w.points[i] += _BA_Point(0.1 * U(gen), 0.1 * U(gen), 0.1 * U(gen));
  return w;
}

static void Register(FullBundleAdjustmentSolverRefactor &s, Scene &w) {
  s.SetVerbose(false);
  OptimizerCamera cam;
  cam.fx = w.cam.fx;
  cam.fy = w.cam.fy;
  cam.cx = w.cam.cx;
  cam.cy = w.cam.cy;
  cam.camera_to_body_pose = w.cam.pose_this_to_cam0;
  s.RegisterCamera(0, cam);
  for (auto &T : w.poses) s.RegisterWorldToBodyPose(&T);
  for (auto &X : w.points) s.RegisterWorldPoint(&X);
  s.MakePoseFixed(&w.poses[0]);
  s.MakePointFixed(&w.points[12]);
  s.MakePointFixed(&w.points[13]);
  for (const auto &o : w.obs) s.AddObservation(0, &w.poses[o.j], &w.points[o.i], o.uv);
}

static void Register(FullBundleAdjustmentSolver &s, Scene &w) {
  s.SetVerbose(false);
  s.AddCamera(0, w.cam);
  for (auto &T : w.poses) s.AddPose(&T);
  for (auto &X : w.points) s.AddPoint(&X);
  s.MakePoseFixed(&w.poses[0]);
  s.MakePointFixed(&w.points[12]);
  s.MakePointFixed(&w.points[13]);
  for (const auto &o : w.obs) s.AddObservation(0, &w.poses[o.j], &w.points[o.i], o.uv);
}

// largest relative block difference between the facade and the converted C-ABI blocks
template <class Solver>
static double Compare(Solver &s, Scene &w, double sigma, int *fail) {
  std::vector<_BA_Pose *> ps = {&w.poses[2], &w.poses[1], &w.poses[2]};
  std::vector<_BA_Point *> qs;
  for (int i = 11; i >= 0; --i) qs.push_back(&w.points[i]);
  std::vector<Eigen::Matrix<double, 6, 6>> cp;
  std::vector<Eigen::Matrix<double, 3, 3>> cq;
  if (!s.ComputeCovariance(ps, qs, sigma, &cp, &cq)) ++*fail;
  if (cp.size() != 3 || cq.size() != 12) return 1.0;
  const int32_t pi[3] = {2, 1, 2};
  int32_t qi[12];
  for (int k = 0; k < 12; ++k) qi[k] = 11 - k;
  std::vector<double> rp(36 * 3), rq(9 * 12);
  int64_t dropped = -1;
  if (ba_covariance(s.GetHandle(), 1.0, 3, pi, rp.data(), 12, qi, rq.data(), &dropped) != 0 || dropped != 0) ++*fail;
  double worst = 0.0;
  for (int k = 0; k < 3; ++k) {
    double scale = 0.0, diff = 0.0;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        const double want = sigma * sigma * 1e-4 * (r < 3 ? 100.0 : 1.0) * (c < 3 ? 100.0 : 1.0) * rp[36 * k + 6 * r + c];
        scale = std::max(scale, std::fabs(want));
        diff = std::max(diff, std::fabs(cp[k](r, c) - want));
      }
    if (!(scale > 0.0)) ++*fail;
    worst = std::max(worst, diff / scale);
  }
  for (int k = 0; k < 12; ++k) {
    double scale = 0.0, diff = 0.0;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        const double want = sigma * sigma * rq[9 * k + 3 * r + c];
        scale = std::max(scale, std::fabs(want));
        diff = std::max(diff, std::fabs(cq[k](r, c) - want));
      }
    if (!(scale > 0.0)) ++*fail;
    worst = std::max(worst, diff / scale);
  }
  // the repeated pose comes back twice, bit for bit
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c)
      if (cp[0](r, c) != cp[2](r, c)) ++*fail;
  return worst;
}

template <class F>
static bool Throws(F f) {
  try {
    f();
  } catch (const std::runtime_error &) {
    return true;
  }
  return false;
}

int main() {
  int fail = 0;
  Scene w = MakeScene();
  FullBundleAdjustmentSolver s;
  Register(s, w);
  const Scene before = w;
  const double e0 = Compare(s, w, 0.7, &fail);
  // the call moves nothing
  for (size_t j = 0; j < w.poses.size(); ++j)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c)
        if (w.poses[j].matrix()(r, c) != before.poses[j].matrix()(r, c)) ++fail;
  Options options;
  options.iteration_handle.max_num_iterations = 8;
  s.Solve(options);
  const double e1 = Compare(s, w, 1.3, &fail);
  std::printf("facade vs C ABI after the unit conversion: max rel err %.2e (start) %.2e (solution)\n", e0, e1);
  if (!(e0 <= 1e-14 && e1 <= 1e-14)) ++fail;
  // an unregistered or fixed pointer throws, as MakePoseFixed does
  _BA_Pose stranger = _BA_Pose::Identity();
  _BA_Point nowhere(0, 0, 1);
  std::vector<Eigen::Matrix<double, 6, 6>> cp;
  std::vector<Eigen::Matrix<double, 3, 3>> cq;
  if (!Throws([&] { s.ComputeCovariance({&stranger}, {}, 1.0, &cp, &cq); })) ++fail;
  if (!Throws([&] { s.ComputeCovariance({}, {&nowhere}, 1.0, &cp, &cq); })) ++fail;
  if (!Throws([&] { s.ComputeCovariance({&w.poses[0]}, {}, 1.0, &cp, &cq); })) ++fail;
  if (!Throws([&] { s.ComputeCovariance({}, {&w.points[13]}, 1.0, &cp, &cq); })) ++fail;
  // the refactored class forwards the call
  Scene w2 = MakeScene();
  FullBundleAdjustmentSolverRefactor r;
  Register(r, w2);
  const double e2 = Compare(r, w2, 1.0, &fail);
  std::printf("refactored class: max rel err %.2e\n", e2);
  if (!(e2 <= 1e-14)) ++fail;
  std::printf(fail ? "COVARIANCE FACADE TEST FAILED (%d)\n" : "COVARIANCE FACADE TEST PASSED\n", fail);
  return fail ? 1 : 0;
}
