// GPU test of the observation mask and the cull on the C++ facade.  Two small windows (stereo
// 5 poses, mono 6 poses; poses 0 and 1 fixed) with a few observations displaced by 40..70
// pixels.  FullBundleAdjustmentSolver::SolveBatch with a CullOptions, in the caller's units,
// must write back the poses and points that ba_batch_solve_culled gives when called directly
// through include/ba_hip.h on the same arrays in scaled units (the facade's preprocessing
// restated here), bit for bit, and report its mask and counts; the `inliers` it reports,
// handed on as obs_masks, must make ComputeCovarianceBatch and MarginalizeBatch return what
// ba_batch_set_obs_mask + ba_batch_covariance / ba_batch_marginalize return, converted as the
// facade converts; obs_masks on SolveBatch is ba_batch_set_obs_mask + ba_batch_solve; malformed
// arguments throw; the refactored class forwards the arguments.  Exit code 0 = pass.
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
using Cull = FullBundleAdjustmentSolver::CullOptions;
using Report = FullBundleAdjustmentSolver::CullReport;
using Masks = std::vector<std::vector<uint8_t>>;

constexpr int kMarked = 2;
constexpr int kFirst = 4, kSecond = 5;

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
  std::vector<uint8_t> displaced;
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
        const _BA_Point Xc = w.cams[c].pose_this_to_cam0 * (truth[j].inverse() * Xt[i]);
        Window::Obs o;
        o.c = c;
        o.j = j;
        o.i = i;
        o.uv = _BA_Pixel(525.0 * Xc(0) / Xc(2) + 320.0, 525.0 * Xc(1) / Xc(2) + 240.0);
        // every 17th observation is an outlier: 40..70 px away
        const bool out = w.obs.size() % 17 == 5;
        if (out) {
          const double ang = 3.14159 * U(gen), mag = 55.0 + 15.0 * U(gen);
          o.uv += _BA_Pixel(mag * std::cos(ang), mag * std::sin(ang));
        }
        w.displaced.push_back(out);
        w.obs.push_back(o);
      }
  w.poses = truth;
  w.fixed_pose.assign(n_pose, 0);
  w.fixed_pose[0] = w.fixed_pose[1] = 1;
  for (int j = 2; j < n_pose; ++j) w.poses[j].translation() += _BA_Point(0.02 * U(gen), 0.02 * U(gen), 0.02 * U(gen));
  w.points = Xt;
  for (int i = 0; i < n_pt; ++i) w.points[i] += _BA_Point(0.05 * U(gen), 0.05 * U(gen), 0.05 * U(gen));
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

// everything the direct calls return, scaled units
struct DirectOut {
  std::vector<double> T, X, cov_pose, cov_pt, H, b;
  std::vector<int64_t> H_off, b_off;
  std::vector<uint8_t> mask, marg_pt;
  std::vector<ba_batch_cull_result> cres;
  std::vector<ba_batch_result> res_first;
};

// mode 0: ba_batch_solve_culled, then covariance and marginalisation of the masked batch at the
// START values (a second batch with the mask set); mode 1: ba_batch_set_obs_mask(given) + solve
static bool Direct(const std::vector<Window> &win, int mode, const Options &first, const Options &second,
                   const ba_cull_options &co, const std::vector<uint8_t> &given, DirectOut *out, Arrays *arr) {
  Arrays a = PackWindows(win);
  const int B = static_cast<int>(win.size());
  const ba_options o1 = MakeOptions(first), o2 = MakeOptions(second);
  ba_handle *h = nullptr;
  ba_batch *batch = nullptr, *fresh = nullptr;
  std::vector<ba_batch_result> res(B);
  out->res_first.resize(B);
  out->cres.resize(B);
  out->T.resize(a.T.size());
  out->X.resize(a.X.size());
  out->mask.assign(a.oc.size(), 7);
  auto create = [&](ba_batch **b) {
    return ba_batch_create(b, h, B, a.cam_off.data(), a.pose_off.data(), a.pt_off.data(), a.obs_off.data(),
                           a.intr.data(), a.T_cj.data(), a.T.data(), a.pose_fixed.data(), a.X.data(),
                           a.point_fixed.data(), a.oc.data(), a.op.data(), a.oq.data(), a.uv.data());
  };
  int rc = ba_create(&h, 0);
  if (rc == 0) rc = create(&batch);
  if (rc == 0 && mode == 0) {
    rc = ba_batch_solve_culled(batch, &o1, &o2, &co, nullptr, 0, out->res_first.data(), res.data(), out->cres.data());
    if (rc == 0) rc = ba_batch_get_obs_mask(batch, out->mask.data());
    // covariance and marginalisation of the start values under that mask
    if (rc == 0) rc = create(&fresh);
    if (rc == 0) rc = ba_batch_set_obs_mask(fresh, out->mask.data());
    std::vector<ba_batch_cov_result> cr(B);
    std::vector<ba_batch_marg_result> mr(B);
    out->cov_pose.resize(36 * a.pose_fixed.size());
    out->cov_pt.resize(9 * a.point_fixed.size());
    out->H_off.resize(B + 1);
    out->b_off.resize(B + 1);
    out->marg_pt.resize(a.point_fixed.size());
    if (rc == 0) rc = ba_batch_covariance(fresh, 1.0, out->cov_pose.data(), out->cov_pt.data(), cr.data());
    if (rc == 0) rc = ba_batch_marg_layout(fresh, a.mark.data(), out->H_off.data(), out->b_off.data());
    if (rc == 0) {
      out->H.resize(out->H_off[B]);
      out->b.resize(out->b_off[B]);
      rc = ba_batch_marginalize(fresh, 1.0, a.mark.data(), out->H.data(), out->b.data(), out->marg_pt.data(), mr.data());
    }
  }
  if (rc == 0 && mode == 1) {
    rc = ba_batch_set_obs_mask(batch, given.data());
    if (rc == 0) rc = ba_batch_solve(batch, &o2, nullptr, 0, res.data());
  }
  if (rc == 0) rc = ba_batch_get_poses(batch, out->T.data());
  if (rc == 0) rc = ba_batch_get_points(batch, out->X.data());
  if (rc) std::printf("direct call failed: %s\n", ba_last_error());
  ba_batch_destroy(fresh);
  ba_batch_destroy(batch);
  ba_destroy(h);
  *arr = a;
  return rc == 0;
}

// largest difference between the solvers' written-back values and direct results (caller's units)
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

struct Solvers {
  std::vector<Window> win;
  std::vector<std::unique_ptr<FullBundleAdjustmentSolver>> own;
  std::vector<FullBundleAdjustmentSolver *> ptrs;
  std::vector<std::vector<_BA_Pose *>> marked;
  explicit Solvers(const std::vector<Window> &start) : win(start) {
    for (size_t k = 0; k < win.size(); ++k) {
      own.emplace_back(new FullBundleAdjustmentSolver());
      Register(*own.back(), win[k]);
      ptrs.push_back(own.back().get());
      marked.push_back({&win[k].poses[kMarked]});
    }
  }
};

int main() {
  const std::vector<Window> start = {MakeWindow(5, 30, true, 1), MakeWindow(6, 26, false, 2)};
  const double sigma = 0.7, s = 0.01;
  Options second;
  second.iteration_handle.max_num_iterations = kSecond;
  second.convergence_handle.threshold_step_size = 0.0;
  second.convergence_handle.threshold_cost_change = 0.0;
  second.outlier_handle.threshold_huber_loss = 0.02;
  second.trust_region_handle.initial_lambda = 1e-3;
  Cull cull;
  cull.first = second;
  cull.first.iteration_handle.max_num_iterations = kFirst;
  cull.chi2 = 25.0 / (sigma * sigma);  // 25 px^2
  const ba_cull_options co{cull.chi2 * sigma * sigma * s * s, 1};
  int fail = 0;
  DirectOut d0, d1;
  Arrays arr;
  if (!Direct(start, 0, cull.first, second, co, {}, &d0, &arr)) ++fail;
  const int B = static_cast<int>(start.size());
  // 1. SolveBatch with cull is ba_batch_solve_culled; the report is its mask and counts
  std::vector<Report> rep;
  Masks inliers;
  if (!fail) {
    Solvers sv(start);
    std::vector<Summary> sums;
    if (!FullBundleAdjustmentSolver::SolveBatch(sv.ptrs, second, &sums, nullptr, sigma, nullptr, nullptr, &cull, &rep)) ++fail;
    const double d = Compare(sv.win, arr, d0.T, d0.X);
    std::printf("facade with cull vs ba_batch_solve_culled: %.2e\n", d);
    if (d != 0.0 || static_cast<int>(rep.size()) != B) ++fail;
    for (int b = 0; b < B && !fail; ++b) {
      const std::vector<uint8_t> want(d0.mask.begin() + arr.obs_off[b], d0.mask.begin() + arr.obs_off[b + 1]);
      int n_out = 0;
      for (size_t k = 0; k < want.size(); ++k) {
        n_out += start[b].displaced[k];
        if (want[k] != (start[b].displaced[k] ? 0 : 1)) ++fail;  // exactly the displaced ones went
      }
      if (rep[b].inliers != want || rep[b].n_culled != d0.cres[b].n_culled || rep[b].n_culled != n_out ||
          rep[b].starved != 0 || rep[b].n_iter_first != kFirst)
        ++fail;
      if (static_cast<int>(sums[b].GetOptimizationInfoList().size()) != kFirst + kSecond) ++fail;
      inliers.push_back(rep[b].inliers);
    }
  }
  // 2. the inliers as obs_masks of the other two entry points, at the start values
  if (!fail) {
    Solvers sv(start);
    std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> cp, cp_all;
    std::vector<std::vector<Eigen::Matrix<double, 3, 3>>> cq;
    if (!FullBundleAdjustmentSolver::ComputeCovarianceBatch(sv.ptrs, sigma, &cp, &cq, nullptr, nullptr, &inliers)) ++fail;
    if (!FullBundleAdjustmentSolver::ComputeCovarianceBatch(sv.ptrs, sigma, &cp_all, nullptr)) ++fail;
    std::vector<Prior> marg, marg_all;
    if (!FullBundleAdjustmentSolver::MarginalizeBatch(sv.ptrs, sv.marked, sigma, &marg, nullptr, nullptr, &inliers)) ++fail;
    if (!FullBundleAdjustmentSolver::MarginalizeBatch(sv.ptrs, sv.marked, sigma, &marg_all)) ++fail;
    double dc = 0.0, dm = 0.0;
    const double s2 = sigma * sigma, k_pose = s2 * s * s, w = 1.0 / (sigma * sigma * s * s);
    for (int b = 0; b < B && !fail; ++b) {
      for (size_t k = 0; k < cp[b].size(); ++k)
        for (int r = 0; r < 6; ++r)
          for (int c = 0; c < 6; ++c) {
            const double dr = r < 3 ? 100.0 : 1.0, dcc = c < 3 ? 100.0 : 1.0;
            dc = std::max(dc, std::abs(cp[b][k](r, c) - k_pose * (dr * d0.cov_pose[36 * (arr.pose_off[b] + k) + 6 * r + c] * dcc)));
          }
      for (size_t k = 0; k < cq[b].size(); ++k)
        for (int r = 0; r < 3; ++r)
          for (int c = 0; c < 3; ++c) dc = std::max(dc, std::abs(cq[b][k](r, c) - s2 * d0.cov_pt[9 * (arr.pt_off[b] + k) + 3 * r + c]));
      const int dim = marg[b].dim;
      if (dim != static_cast<int>(d0.b_off[b + 1] - d0.b_off[b])) ++fail;
      const auto di = [s](int r) { return r % 6 < 3 ? s : 1.0; };
      for (int r = 0; r < dim && !fail; ++r) {
        for (int c = 0; c < dim; ++c)
          dm = std::max(dm, std::abs(marg[b](r, c) - w * (di(r) * d0.H[d0.H_off[b] + static_cast<size_t>(r) * dim + c] * di(c))));
        dm = std::max(dm, std::abs(marg[b].b[r] - w * (di(r) * d0.b[d0.b_off[b] + r])));
      }
      if (cp[b][3] == cp_all[b][3] || marg[b].H == marg_all[b].H) ++fail;  // the mask is felt
    }
    std::printf("obs_masks: covariance vs direct %.2e, marginalisation vs direct %.2e\n", dc, dm);
    if (dc != 0.0 || dm != 0.0) ++fail;
  }
  // 3. obs_masks on SolveBatch is ba_batch_set_obs_mask + ba_batch_solve; an empty vector is all on
  if (!fail) {
    Masks some = inliers;
    some[1].clear();
    std::vector<uint8_t> flat(d0.mask.begin(), d0.mask.begin() + arr.obs_off[1]);
    flat.resize(d0.mask.size(), 1);
    if (!Direct(start, 1, cull.first, second, co, flat, &d1, &arr)) ++fail;
    Solvers sv(start);
    if (!FullBundleAdjustmentSolver::SolveBatch(sv.ptrs, second, nullptr, nullptr, sigma, nullptr, &some)) ++fail;
    const double d = Compare(sv.win, arr, d1.T, d1.X);
    std::printf("facade with obs_masks vs ba_batch_set_obs_mask + ba_batch_solve: %.2e\n", d);
    if (d != 0.0) ++fail;
    // malformed arguments throw before anything is solved
    Masks bad = inliers;
    bad[0].pop_back();
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(sv.ptrs, second, nullptr, nullptr, sigma, nullptr, &bad); })) ++fail;
    std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> cp;
    if (!Throws([&] { FullBundleAdjustmentSolver::ComputeCovarianceBatch(sv.ptrs, sigma, &cp, nullptr, nullptr, nullptr, &bad); })) ++fail;
    std::vector<Prior> mp;
    if (!Throws([&] { FullBundleAdjustmentSolver::MarginalizeBatch(sv.ptrs, sv.marked, sigma, &mp, nullptr, nullptr, &bad); })) ++fail;
    bad = inliers;
    bad.pop_back();
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(sv.ptrs, second, nullptr, nullptr, sigma, nullptr, &bad); })) ++fail;
    Cull zero = cull;
    zero.chi2 = 0.0;
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(sv.ptrs, second, nullptr, nullptr, sigma, nullptr, nullptr, &zero); })) ++fail;
    Cull idle = cull;
    idle.first.iteration_handle.max_num_iterations = 0;
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(sv.ptrs, second, nullptr, nullptr, sigma, nullptr, nullptr, &idle); })) ++fail;
  }
  // 4. the refactored class forwards the arguments
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
    const Masks one = {inliers[1]};
    std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> cp, cp0;
    if (!FullBundleAdjustmentSolverRefactor::ComputeCovarianceBatch({&r}, sigma, &cp, nullptr, nullptr, nullptr, &one)) ++fail;
    if (!FullBundleAdjustmentSolverRefactor::ComputeCovarianceBatch({&r}, sigma, &cp0, nullptr)) ++fail;
    std::vector<Prior> m1, m0;
    if (!FullBundleAdjustmentSolverRefactor::MarginalizeBatch({&r}, {{&w.poses[kMarked]}}, sigma, &m1, nullptr, nullptr, &one)) ++fail;
    if (!FullBundleAdjustmentSolverRefactor::MarginalizeBatch({&r}, {{&w.poses[kMarked]}}, sigma, &m0)) ++fail;
    if (!fail && (cp[0][3] == cp0[0][3] || m1[0].H == m0[0].H)) ++fail;
    std::vector<FullBundleAdjustmentSolverRefactor::CullReport> rr;
    const FullBundleAdjustmentSolverRefactor::CullOptions rc = cull;
    if (!FullBundleAdjustmentSolverRefactor::SolveBatch({&r}, second, nullptr, nullptr, sigma, nullptr, nullptr, &rc, &rr)) ++fail;
    if (!fail && (rr.size() != 1 || rr[0].inliers != inliers[1] || rr[0].n_culled != rep[1].n_culled)) ++fail;
  }
  std::printf(fail ? "BATCH OBS FACADE TEST FAILED (%d)\n" : "BATCH OBS FACADE TEST PASSED\n", fail);
  return fail ? 1 : 0;
}
