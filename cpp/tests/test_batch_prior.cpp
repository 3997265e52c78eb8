// GPU test of the pose prior on the C++ facade: FullBundleAdjustmentSolver::SolveBatch with
// in_priors.  Two small windows (stereo 5 poses, mono 6 poses; poses 0 and 1 fixed); the
// prior of each is what MarginalizeBatch returns for its oldest optimisable pose, handed back
// as a PosePrior on the kept poses (linearised at the current values, c = 3 in the caller's
// units).  SolveBatch with those priors, in the caller's units, must write back the poses and
// points that ba_batch_set_prior + ba_batch_solve give when called directly through
// include/ba_hip.h on the same arrays in scaled units (the facade's preprocessing restated
// here), bit for bit: the two paths run the same kernel on the same numbers.  The prior must
// matter, the poses of a PosePrior may come in any order, malformed priors throw, and the
// refactored class forwards the argument.  Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <memory>
#include <random>
#include <stdexcept>
#include <vector>

#include "ba_hip.h"
#include "core/full_bundle_adjustment_solver.h"
#include "core/full_bundle_adjustment_solver_refactor.h"
#include "eigen3/Eigen/Dense"

using namespace visual_navigation::analytic_solver;
using Prior = FullBundleAdjustmentSolver::MarginalPrior;

constexpr int kMarked = 2, kSeen = 18;  // the marked pose and the landmarks it observes

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

static Window MakeWindow(int n_pose, int n_pt, bool stereo, unsigned seed) {
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
        if (j == kMarked && i >= kSeen) continue;
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
  for (int i = 0; i < n_pt; ++i) w.points[i] += _BA_Point(0.15 * U(gen), 0.15 * U(gen), 0.15 * U(gen));
  return w;
}

static void Register(FullBundleAdjustmentSolver &s, Window &w) {
  s.SetVerbose(false);
  for (size_t c = 0; c < w.cams.size(); ++c) s.AddCamera(static_cast<int>(c), w.cams[c]);
  for (auto &T : w.poses) s.AddPose(&T);
  for (auto &X : w.points) s.AddPoint(&X);
  for (size_t j = 0; j < w.poses.size(); ++j)
    if (w.fixed_pose[j]) s.MakePoseFixed(&w.poses[j]);
  for (const auto &o : w.obs) s.AddObservation(o.c, &w.poses[o.j], &w.points[o.i], o.uv);
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


using InPrior = FullBundleAdjustmentSolver::PosePrior;
constexpr double kC = 3.0;  // the priors' constant, caller's units
constexpr int kIters = 4;

struct Arrays {
  std::vector<int32_t> cam_off{0}, pose_off{0}, pt_off{0}, oc, op, oq;
  std::vector<int64_t> obs_off{0};
  std::vector<double> intr, T_cj, T, X, uv;
  std::vector<uint8_t> pose_fixed, point_fixed, mark;
};

static void Pack(const _BA_Pose &P, std::vector<double> &v) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) v.push_back(P.linear()(r, c));
  for (int r = 0; r < 3; ++r) v.push_back(P.translation()(r));
}

static Arrays PackWindows(const std::vector<Window> &win) {
  const double s = 0.01;
  Arrays a;
  for (const Window &w : win) {
    for (const _BA_Camera &cam : w.cams) {
      a.intr.insert(a.intr.end(), {cam.fx * s, cam.fy * s, cam.cx * s, cam.cy * s});
      _BA_Pose P = cam.pose_this_to_cam0;
      P.translation() *= s;
      Pack(P, a.T_cj);
    }
    for (size_t j = 0; j < w.poses.size(); ++j) {
      _BA_Pose P = w.poses[j].inverse();
      P.translation() = P.translation() * s;
      Pack(P, a.T);
      a.pose_fixed.push_back(static_cast<uint8_t>(w.fixed_pose[j]));
      a.mark.push_back(static_cast<int>(j) == kMarked);
    }
    for (const _BA_Point &Q : w.points) {
      const _BA_Point Qs = Q * s;
      for (int r = 0; r < 3; ++r) a.X.push_back(Qs(r));
      a.point_fixed.push_back(0);
    }
    for (const auto &o : w.obs) {
      a.oc.push_back(o.c);
      a.op.push_back(o.j);
      a.oq.push_back(o.i);
      a.uv.push_back(o.uv(0) * s);
      a.uv.push_back(o.uv(1) * s);
    }
    a.cam_off.push_back(static_cast<int32_t>(a.intr.size() / 4));
    a.pose_off.push_back(static_cast<int32_t>(a.pose_fixed.size()));
    a.pt_off.push_back(static_cast<int32_t>(a.point_fixed.size()));
    a.obs_off.push_back(static_cast<int64_t>(a.oc.size()));
  }
  return a;
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

// marginalize, set the result as the prior of the kept poses, solve: all through ba_hip.h.
// with_prior = false: the plain solve.  T / X: the solved values, scaled units.
static bool Direct(const std::vector<Window> &win, double sigma, const Options &options, bool with_prior,
                   std::vector<double> *T, std::vector<double> *X, Arrays *arr) {
  const double s = 0.01;
  Arrays a = PackWindows(win);
  const int B = static_cast<int>(win.size());
  ba_handle *h = nullptr;
  ba_batch *batch = nullptr;
  std::vector<int64_t> H_off(B + 1), b_off(B + 1);
  std::vector<ba_batch_marg_result> mres(B);
  std::vector<ba_batch_result> res(B);
  std::vector<double> H, bv;
  int rc = ba_create(&h, 0);
  if (rc == 0)
    rc = ba_batch_create(&batch, h, B, a.cam_off.data(), a.pose_off.data(), a.pt_off.data(), a.obs_off.data(),
                         a.intr.data(), a.T_cj.data(), a.T.data(), a.pose_fixed.data(), a.X.data(),
                         a.point_fixed.data(), a.oc.data(), a.op.data(), a.oq.data(), a.uv.data());
  if (rc == 0 && with_prior) {
    rc = ba_batch_marg_layout(batch, a.mark.data(), H_off.data(), b_off.data());
    if (rc == 0) {
      H.resize(H_off[B]);
      bv.resize(b_off[B]);
      rc = ba_batch_marginalize(batch, 1.0, a.mark.data(), H.data(), bv.data(), nullptr, mres.data());
    }
    // to the caller's units as MarginalizeBatch converts, and back as SolveBatch converts
    const double wgt = 1.0 / (sigma * sigma * s * s), inv = 100.0;
    std::vector<int32_t> off{0}, pose;
    std::vector<double> Tl, cs;
    for (int b = 0; b < B && rc == 0; ++b) {
      const int dim = static_cast<int>(b_off[b + 1] - b_off[b]);
      for (int r = 0; r < dim; ++r) {
        const double dr = r % 6 < 3 ? s : 1.0, ir = r % 6 < 3 ? inv : 1.0;
        for (int c = 0; c < dim; ++c) {
          double &v = H[H_off[b] + static_cast<size_t>(r) * dim + c];
          v = wgt * (dr * v * (c % 6 < 3 ? s : 1.0));
          v = (ir * v * (c % 6 < 3 ? inv : 1.0)) / wgt;
        }
        double &u = bv[b_off[b] + r];
        u = wgt * (dr * u);
        u = (ir * u) / wgt;
      }
      for (size_t j = 0; j < win[b].poses.size(); ++j)
        if (!win[b].fixed_pose[j] && static_cast<int>(j) != kMarked) {
          pose.push_back(static_cast<int32_t>(j));
          const double *src = &a.T[12 * (static_cast<size_t>(a.pose_off[b]) + j)];
          Tl.insert(Tl.end(), src, src + 12);
        }
      off.push_back(static_cast<int32_t>(pose.size()));
      cs.push_back(kC / wgt);
    }
    if (rc == 0) rc = ba_batch_prior_check(B, a.pose_off.data(), a.pose_fixed.data(), off.data(), pose.data(), Tl.data(),
                                           H.data(), bv.data(), cs.data());
    if (rc == 0) rc = ba_batch_set_prior(batch, off.data(), pose.data(), Tl.data(), H.data(), bv.data(), cs.data());
    int64_t info[4] = {0, 0, 0, 0};
    if (rc == 0) rc = ba_batch_prior_info(batch, info);
    if (rc == 0 && (info[0] != B || info[1] != static_cast<int64_t>(pose.size()) || info[2] <= 0)) {
      std::printf("ba_batch_prior_info: %lld %lld %lld\n", (long long)info[0], (long long)info[1], (long long)info[2]);
      rc = -2;
    }
  }
  const ba_options o = MakeOptions(options);
  if (rc == 0) rc = ba_batch_solve(batch, &o, nullptr, 0, res.data());
  T->resize(a.T.size());
  X->resize(a.X.size());
  if (rc == 0) rc = ba_batch_get_poses(batch, T->data());
  if (rc == 0) rc = ba_batch_get_points(batch, X->data());
  if (rc == -1) std::printf("direct call failed: %s\n", ba_last_error());
  ba_batch_destroy(batch);
  ba_destroy(h);
  for (int b = 0; b < B && rc == 0; ++b)
    if (res[b].status != 0 || res[b].n_iter != kIters) rc = -3;
  *arr = a;
  return rc == 0;
}

// max |facade value - direct value converted as WriteBack converts|; 0 = the same bits
static double Compare(const std::vector<Window> &win, const Arrays &a, const std::vector<double> &T,
                      const std::vector<double> &X) {
  double diff = 0.0;
  for (size_t k = 0; k < win.size(); ++k) {
    for (size_t j = 0; j < win[k].poses.size(); ++j) {
      if (win[k].fixed_pose[j]) continue;
      const double *src = &T[12 * (static_cast<size_t>(a.pose_off[k]) + j)];
      _BA_Pose P;
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P.linear()(r, c) = src[3 * r + c];
        P.translation()(r) = src[9 + r];
      }
      P.translation() *= 100.0;
      const _BA_Pose Q = P.inverse();
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c)
          diff = std::max(diff, std::fabs(Q.linear()(r, c) - win[k].poses[j].linear()(r, c)));
        diff = std::max(diff, std::fabs(Q.translation()(r) - win[k].poses[j].translation()(r)));
      }
    }
    for (size_t i = 0; i < win[k].points.size(); ++i) {
      const double *src = &X[3 * (static_cast<size_t>(a.pt_off[k]) + i)];
      const _BA_Point Q = _BA_Point(src[0], src[1], src[2]) * 100.0;
      for (int r = 0; r < 3; ++r) diff = std::max(diff, std::fabs(Q(r) - win[k].points[i](r)));
    }
  }
  return diff;
}

int main() {
  const std::vector<Window> start = {MakeWindow(5, 30, true, 1), MakeWindow(6, 26, false, 2)};
  const double sigma = 0.7;
  Options options;
  options.iteration_handle.max_num_iterations = kIters;
  options.convergence_handle.threshold_step_size = 0.0;
  options.convergence_handle.threshold_cost_change = 0.0;
  int fail = 0;
  std::vector<double> T_prior, X_prior, T_free, X_free;
  Arrays arr;
  if (!Direct(start, sigma, options, true, &T_prior, &X_prior, &arr)) ++fail;
  if (!Direct(start, sigma, options, false, &T_free, &X_free, &arr)) ++fail;
  for (int reversed = 0; reversed < 2 && !fail; ++reversed) {
    std::vector<Window> win = start;
    std::vector<std::unique_ptr<FullBundleAdjustmentSolver>> own;
    std::vector<FullBundleAdjustmentSolver *> ptrs;
    std::vector<std::vector<_BA_Pose *>> marked;
    for (size_t k = 0; k < win.size(); ++k) {
      own.emplace_back(new FullBundleAdjustmentSolver());
      Register(*own.back(), win[k]);
      ptrs.push_back(own.back().get());
      marked.push_back({&win[k].poses[kMarked]});
    }
    std::vector<Prior> marg;
    if (!FullBundleAdjustmentSolver::MarginalizeBatch(ptrs, marked, sigma, &marg)) ++fail;
    std::vector<InPrior> in;
    for (const Prior &m : marg) in.emplace_back(m, kC);
    if (reversed)  // the same priors with their poses (and blocks) in reverse order
      for (InPrior &p : in) {
        const int K = static_cast<int>(p.poses.size()), n = 6 * K;
        InPrior q = p;
        for (int t = 0; t < K; ++t) {
          q.poses[t] = p.poses[K - 1 - t];
          q.lin_poses[t] = p.lin_poses[K - 1 - t];
        }
        for (int r = 0; r < n; ++r) {
          const int sr = 6 * (K - 1 - r / 6) + r % 6;
          q.b[r] = p.b[sr];
          for (int c = 0; c < n; ++c) q.H[static_cast<size_t>(r) * n + c] = p.H[static_cast<size_t>(sr) * n + 6 * (K - 1 - c / 6) + c % 6];
        }
        p = q;
      }
    if (!FullBundleAdjustmentSolver::SolveBatch(ptrs, options, nullptr, &in, sigma)) ++fail;
    const double d_prior = Compare(win, arr, T_prior, X_prior), d_free = Compare(win, arr, T_free, X_free);
    std::printf("%s: facade with priors vs direct call with the prior %.2e, vs direct call without %.2e\n",
                reversed ? "reversed pose order" : "registration order", d_prior, d_free);
    if (!(d_prior == 0.0 && d_free > 1e-9)) ++fail;
    if (reversed) continue;
    // the other two entry points take the argument; malformed priors throw
    std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> cp, cp0;
    if (!FullBundleAdjustmentSolver::ComputeCovarianceBatch(ptrs, sigma, &cp, nullptr, &in)) ++fail;
    if (!FullBundleAdjustmentSolver::ComputeCovarianceBatch(ptrs, sigma, &cp0, nullptr)) ++fail;
    if (!fail && !(cp[0][3](0, 0) > 0.0 && cp[0][3](0, 0) < cp0[0][3](0, 0))) ++fail;  // information was added
    std::vector<Prior> chained;
    if (!FullBundleAdjustmentSolver::MarginalizeBatch(ptrs, marked, sigma, &chained, &in)) ++fail;
    if (!fail && (chained[0].dim != marg[0].dim || chained[0].H == marg[0].H)) ++fail;
    std::vector<InPrior> bad = in;
    bad[0].b.pop_back();
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(ptrs, options, nullptr, &bad, sigma); })) ++fail;
    bad = in;
    _BA_Pose stranger = _BA_Pose::Identity();
    bad[1].poses[0] = &stranger;
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(ptrs, options, nullptr, &bad, sigma); })) ++fail;
    bad = in;
    bad.pop_back();
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(ptrs, options, nullptr, &bad, sigma); })) ++fail;
    bad = in;
    bad[0].poses[0] = &win[0].poses[0];  // a fixed pose: refused by the library before the GPU is touched
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(ptrs, options, nullptr, &bad, sigma); })) ++fail;
  }
  // the refactored class forwards the argument
  if (!fail) {
    Window w = start[1];
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
    std::vector<Prior> m0, m1;
    if (!FullBundleAdjustmentSolverRefactor::MarginalizeBatch({&r}, {{&w.poses[kMarked]}}, sigma, &m0)) ++fail;
    std::vector<InPrior> in;
    for (const Prior &m : m0) in.emplace_back(m, kC);
    if (!FullBundleAdjustmentSolverRefactor::MarginalizeBatch({&r}, {{&w.poses[kMarked]}}, sigma, &m1, &in)) ++fail;
    std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> cp, cp0;
    if (!FullBundleAdjustmentSolverRefactor::ComputeCovarianceBatch({&r}, sigma, &cp, nullptr, &in)) ++fail;
    if (!FullBundleAdjustmentSolverRefactor::ComputeCovarianceBatch({&r}, sigma, &cp0, nullptr)) ++fail;
    if (!fail && (m1[0].H == m0[0].H || !(cp[0][3](0, 0) < cp0[0][3](0, 0)))) ++fail;
  }
  std::printf(fail ? "BATCH PRIOR FACADE TEST FAILED (%d)\n" : "BATCH PRIOR FACADE TEST PASSED\n", fail);
  return fail ? 1 : 0;
}
