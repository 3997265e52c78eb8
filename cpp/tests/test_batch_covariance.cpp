// GPU test of FullBundleAdjustmentSolver::ComputeCovarianceBatch: three small windows
// (stereo 5 poses, mono 4 poses, stereo 6 poses with a fixed point; the windows of
// test_full_batch.cpp) get their covariance blocks once by ONE ComputeCovarianceBatch and
// once by ComputeCovariance on each solver's own handle.  Every block of a free member must
// agree to 2e-11 relative (largest element difference over the block's largest element):
// each path lies within 1e-11 of the host inverse at the noise floor of these stereo /
// two-fixed-pose windows, and 2e-11 is the sum.  Blocks of fixed members are zero, a
// sharded solver throws, the refactored class forwards the call.  Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <memory>
#include <random>
#include <stdexcept>
#include <vector>

#include "core/full_bundle_adjustment_solver.h"
#include "core/full_bundle_adjustment_solver_refactor.h"
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

template <class M>
static double RelBlock(const M &a, const M &b) {
  double scale = 0.0, diff = 0.0;
  for (int r = 0; r < a.rows(); ++r)
    for (int c = 0; c < a.cols(); ++c) {
      scale = std::max(scale, std::fabs(b(r, c)));
      diff = std::max(diff, std::fabs(a(r, c) - b(r, c)));
    }
  return scale > 0.0 ? diff / scale : (diff == 0.0 ? 0.0 : 1.0);
}

template <class M>
static bool IsZero(const M &a) {
  for (int r = 0; r < a.rows(); ++r)
    for (int c = 0; c < a.cols(); ++c)
      if (a(r, c) != 0.0) return false;
  return true;
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
  std::vector<Window> win = {MakeWindow(5, 30, true, 1, -1), MakeWindow(4, 26, false, 2, -1),
                             MakeWindow(6, 34, true, 3, 7)};
  const double sigma = 0.7;
  std::vector<std::unique_ptr<FullBundleAdjustmentSolver>> own;
  std::vector<FullBundleAdjustmentSolver *> ptrs;
  for (size_t k = 0; k < win.size(); ++k) {
    own.emplace_back(new FullBundleAdjustmentSolver());
    Register(*own.back(), win[k]);
    ptrs.push_back(own.back().get());
  }
  std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> bp;
  std::vector<std::vector<Eigen::Matrix<double, 3, 3>>> bq;
  int fail = FullBundleAdjustmentSolver::ComputeCovarianceBatch(ptrs, sigma, &bp, &bq) ? 0 : 1;
  if (bp.size() != win.size() || bq.size() != win.size()) ++fail;
  for (size_t k = 0; k < win.size() && !fail; ++k) {
    Window &w = win[k];
    if (bp[k].size() != w.poses.size() || bq[k].size() != w.points.size()) {
      ++fail;
      break;
    }
    // the handle path: every free member of this solver
    std::vector<_BA_Pose *> ps;
    std::vector<_BA_Point *> qs;
    std::vector<size_t> pj, qi;
    for (size_t j = 0; j < w.poses.size(); ++j)
      if (!w.fixed_pose[j]) {
        ps.push_back(&w.poses[j]);
        pj.push_back(j);
      } else if (!IsZero(bp[k][j])) {
        ++fail;
      }
    for (size_t i = 0; i < w.points.size(); ++i)
      if (!w.fixed_point[i]) {
        qs.push_back(&w.points[i]);
        qi.push_back(i);
      } else if (!IsZero(bq[k][i])) {
        ++fail;
      }
    std::vector<Eigen::Matrix<double, 6, 6>> hp;
    std::vector<Eigen::Matrix<double, 3, 3>> hq;
    if (!ptrs[k]->ComputeCovariance(ps, qs, sigma, &hp, &hq)) ++fail;
    if (hp.size() != ps.size() || hq.size() != qs.size()) {
      ++fail;
      break;
    }
    double ep = 0.0, eq = 0.0;
    for (size_t t = 0; t < pj.size(); ++t) {
      ep = std::max(ep, RelBlock(bp[k][pj[t]], hp[t]));
      if (!(bp[k][pj[t]](0, 0) > 0.0)) ++fail;
    }
    for (size_t t = 0; t < qi.size(); ++t) eq = std::max(eq, RelBlock(bq[k][qi[t]], hq[t]));
    std::printf("window %zu: batch vs handle path, max rel block diff pose %.2e point %.2e\n", k, ep, eq);
    if (!(ep <= 2e-11 && eq <= 2e-11)) ++fail;
  }
  // pose blocks alone
  std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> bp2;
  if (!FullBundleAdjustmentSolver::ComputeCovarianceBatch(ptrs, sigma, &bp2, nullptr)) ++fail;
  for (size_t k = 0; k < win.size() && !fail; ++k)
    for (size_t j = 0; j < bp[k].size(); ++j)
      if (RelBlock(bp2[k][j], bp[k][j]) != 0.0) ++fail;
  // a sharded solver cannot join a batch
  {
    Window w = win[0];
    FullBundleAdjustmentSolver sharded;
    Register(sharded, w);
    sharded.SetShard(0, 2);
    std::vector<FullBundleAdjustmentSolver *> mix = {ptrs[0], &sharded};
    if (!Throws([&] { FullBundleAdjustmentSolver::ComputeCovarianceBatch(mix, sigma, &bp2, nullptr); })) ++fail;
  }
  // the refactored class forwards the call
  {
    Window w = win[1];
    FullBundleAdjustmentSolverRefactor r;
    r.SetVerbose(false);
    OptimizerCamera cam;
    cam.fx = w.cams[0].fx;
    cam.fy = w.cams[0].fy;
    cam.cx = w.cams[0].cx;
    cam.cy = w.cams[0].cy;
    cam.camera_to_body_pose = w.cams[0].pose_this_to_cam0;
    r.RegisterCamera(0, cam);
    for (auto &T : w.poses) r.RegisterWorldToBodyPose(&T);
    for (auto &X : w.points) r.RegisterWorldPoint(&X);
    for (size_t j = 0; j < w.poses.size(); ++j)
      if (w.fixed_pose[j]) r.MakePoseFixed(&w.poses[j]);
    for (const auto &o : w.obs) r.AddObservation(0, &w.poses[o.j], &w.points[o.i], o.uv);
    std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> rp;
    std::vector<std::vector<Eigen::Matrix<double, 3, 3>>> rq;
    if (!FullBundleAdjustmentSolverRefactor::ComputeCovarianceBatch({&r}, sigma, &rp, &rq)) ++fail;
    if (rp.size() != 1 || rp[0].size() != bp[1].size()) {
      ++fail;
    } else {
      for (size_t j = 0; j < rp[0].size(); ++j)
        if (RelBlock(rp[0][j], bp[1][j]) != 0.0) ++fail;
    }
  }
  std::printf(fail ? "BATCH COVARIANCE FACADE TEST FAILED (%d)\n" : "BATCH COVARIANCE FACADE TEST PASSED\n", fail);
  return fail ? 1 : 0;
}
