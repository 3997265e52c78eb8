// GPU test of the relative-pose factors on the C++ facades: SolveBatch, ComputeCovarianceBatch
// and MarginalizeBatch with in_relatives.  Two small windows (stereo 5 poses, mono 6 poses; poses
// 0 and 1 fixed) carry an odometry chain over consecutive poses (its first factor ends on a
// fixed pose) and one loop closure.  SolveBatch with the factors in the caller's units must
// write back the poses and points that ba_batch_set_relative + ba_batch_solve give when called
// directly through include/ba_hip.h on the same arrays in scaled units (the facade's
// preprocessing restated here), bit for bit.  Then the chain of a sliding window: SolveBatch ->
// MarginalizeBatch of the oldest optimisable pose (the factors that name it leave with it) ->
// SolveBatch of the reduced window with the returned prior and the factors that stayed.  The
// refactored class runs the same chain and must end on the same bits.  Exit code 0 = pass.
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
using Rel = FullBundleAdjustmentSolver::RelativePose;
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


// the factors of one window: the chain (q + 1, q) from pose 1 on and the loop closure
// (n - 1, 2); the measurement is the relative pose of the start values moved by a centimetre,
// the information the caller's-units image of diag(2e4 I3, 2e2 I3) plus one off-diagonal pair
static std::vector<Rel> MakeFactors(Window &w, double sigma) {
  const int n = static_cast<int>(w.poses.size());
  std::vector<std::pair<int, int>> pairs;
  for (int q = 1; q + 1 < n; ++q) pairs.emplace_back(q + 1, q);
  pairs.emplace_back(n - 1, 2);
  const double wgt = 1.0 / (sigma * sigma * 1e-4);
  std::vector<Rel> out;
  for (size_t f = 0; f < pairs.size(); ++f) {
    Rel r;
    r.pose_j = &w.poses[pairs[f].first];
    r.pose_k = &w.poses[pairs[f].second];
    r.measurement = r.pose_j->inverse() * (*r.pose_k);
    r.measurement.translation() += _BA_Point(0.01, -0.005 * (1.0 + f), 0.008);
    for (int a = 0; a < 6; ++a) {
      const double da = a < 3 ? 0.01 : 1.0;  // marginal_to_user_units: H_u = w D^-1 H D^-1, D = diag(100 I3, I3)
      r.information[6 * a + a] = wgt * da * (a < 3 ? 2e4 : 2e2) * da;
    }
    r.information[6 * 4 + 1] = r.information[6 * 1 + 4] = wgt * 0.01 * 3e2;
    out.push_back(r);
  }
  return out;
}

// the same factors in scaled units, as PackRelatives converts them
struct RelArrays {
  std::vector<int32_t> off{0}, j, k;
  std::vector<double> Z, Om;
};

static RelArrays PackFactors(const std::vector<Window> &win, const std::vector<std::vector<Rel>> &rels, double sigma) {
  const double s = 0.01, inv = 100.0, wgt = 1.0 / (sigma * sigma * s * s);
  RelArrays a;
  for (size_t b = 0; b < win.size(); ++b) {
    for (const Rel &r : rels[b]) {
      a.j.push_back(static_cast<int32_t>(r.pose_j - &win[b].poses[0]));
      a.k.push_back(static_cast<int32_t>(r.pose_k - &win[b].poses[0]));
      _BA_Pose Z = r.measurement;
      Z.translation() = Z.translation() * s;
      Pack(Z, a.Z);
      for (int rr = 0; rr < 6; ++rr)
        for (int c = 0; c < 6; ++c)
          a.Om.push_back(((rr < 3 ? inv : 1.0) * r.information[6 * rr + c] * (c < 3 ? inv : 1.0)) / wgt);
    }
    a.off.push_back(static_cast<int32_t>(a.j.size()));
  }
  return a;
}

// ba_batch_set_relative + ba_batch_solve through ba_hip.h; with_rel = false: the plain solve
static bool Direct(const std::vector<Window> &win, const std::vector<std::vector<Rel>> &rels, double sigma,
                   const Options &options, bool with_rel, std::vector<double> *T, std::vector<double> *X, Arrays *arr) {
  Arrays a = PackWindows(win);
  const RelArrays ra = PackFactors(win, rels, sigma);
  const int B = static_cast<int>(win.size());
  ba_handle *h = nullptr;
  ba_batch *batch = nullptr;
  std::vector<ba_batch_result> res(B);
  int rc = ba_create(&h, 0);
  if (rc == 0)
    rc = ba_batch_create(&batch, h, B, a.cam_off.data(), a.pose_off.data(), a.pt_off.data(), a.obs_off.data(),
                         a.intr.data(), a.T_cj.data(), a.T.data(), a.pose_fixed.data(), a.X.data(),
                         a.point_fixed.data(), a.oc.data(), a.op.data(), a.oq.data(), a.uv.data());
  if (rc == 0 && with_rel) {
    rc = ba_batch_relative_check(B, a.pose_off.data(), a.pose_fixed.data(), ra.off.data(), ra.j.data(), ra.k.data(),
                                 ra.Z.data(), ra.Om.data());
    if (rc == 0) rc = ba_batch_set_relative(batch, ra.off.data(), ra.j.data(), ra.k.data(), ra.Z.data(), ra.Om.data());
    int64_t info[4] = {0, 0, 0, 0};
    if (rc == 0) rc = ba_batch_relative_info(batch, info);
    if (rc == 0 && (info[0] != B || info[1] != static_cast<int64_t>(ra.j.size()) || info[2] <= 0)) rc = -2;
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


// the reduced window on the same storage: every pose but the marked one, every point that did
// not leave, the observations among them
template <class Solver, class AddPoseFn, class AddPointFn>
static void RegisterReduced(Solver &s, Window &w, const Prior &m, AddPoseFn add_pose, AddPointFn add_point) {
  std::vector<char> gone(w.points.size(), 0);
  for (const _BA_Point *q : m.marginalized_points) gone[static_cast<size_t>(q - &w.points[0])] = 1;
  for (size_t j = 0; j < w.poses.size(); ++j)
    if (static_cast<int>(j) != kMarked) add_pose(&w.poses[j]);
  for (size_t i = 0; i < w.points.size(); ++i)
    if (!gone[i]) add_point(&w.points[i]);
  for (size_t j = 0; j < w.poses.size(); ++j)
    if (w.fixed_pose[j]) s.MakePoseFixed(&w.poses[j]);
  for (const auto &o : w.obs)
    if (o.j != kMarked && !gone[static_cast<size_t>(o.i)]) s.AddObservation(o.c, &w.poses[o.j], &w.points[o.i], o.uv);
}

static std::vector<Rel> Stayed(const std::vector<Rel> &rels, const Prior &m) {
  std::vector<Rel> out;
  for (size_t f = 0; f < rels.size(); ++f)
    if (!m.relatives_left[f]) out.push_back(rels[f]);
  return out;
}

// which factors must leave with the marked pose
static bool LeftAsExpected(const Window &w, const std::vector<Rel> &rels, const Prior &m) {
  if (m.relatives_left.size() != rels.size()) return false;
  int left = 0;
  for (size_t f = 0; f < rels.size(); ++f) {
    const bool names = rels[f].pose_j == &w.poses[kMarked] || rels[f].pose_k == &w.poses[kMarked];
    if ((m.relatives_left[f] != 0) != names) return false;
    left += names;
  }
  return left == 3 && left < static_cast<int>(rels.size());  // (2, 1), (3, 2) and the loop closure (n - 1, 2)
}

static void RegisterRefactor(FullBundleAdjustmentSolverRefactor &r, Window &w) {
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
}

int main() {
  const std::vector<Window> start = {MakeWindow(5, 30, true, 1), MakeWindow(6, 26, false, 2)};
  const double sigma = 0.7;
  Options options;
  options.solver_type = SolverType::LEVENBERG_MARQUARDT;  // the refactored class selects by it
  options.iteration_handle.max_num_iterations = kIters;
  options.convergence_handle.threshold_step_size = 0.0;
  options.convergence_handle.threshold_cost_change = 0.0;
  int fail = 0;
  std::vector<Window> base = start;  // the windows the first class works on; the factors point into them
  std::vector<std::vector<Rel>> rels;
  for (Window &w : base) rels.push_back(MakeFactors(w, sigma));
  std::vector<double> T_rel, X_rel, T_free, X_free;
  Arrays arr;
  if (!Direct(base, rels, sigma, options, true, &T_rel, &X_rel, &arr)) ++fail;
  if (!Direct(base, rels, sigma, options, false, &T_free, &X_free, &arr)) ++fail;
  // ---- FullBundleAdjustmentSolver: solve, marginalise, solve the reduced window -----------
  std::vector<Prior> marg, marg0;
  if (!fail) {
    std::vector<std::unique_ptr<FullBundleAdjustmentSolver>> own;
    std::vector<FullBundleAdjustmentSolver *> ptrs;
    std::vector<std::vector<_BA_Pose *>> marked;
    for (size_t k = 0; k < base.size(); ++k) {
      own.emplace_back(new FullBundleAdjustmentSolver());
      Register(*own.back(), base[k]);
      ptrs.push_back(own.back().get());
      marked.push_back({&base[k].poses[kMarked]});
    }
    if (!FullBundleAdjustmentSolver::SolveBatch(ptrs, options, nullptr, nullptr, sigma, &rels)) ++fail;
    const double d_rel = Compare(base, arr, T_rel, X_rel), d_free = Compare(base, arr, T_free, X_free);
    std::printf("facade with factors vs direct call with them %.2e, vs direct call without %.2e\n", d_rel, d_free);
    if (!(d_rel == 0.0 && d_free > 1e-9)) ++fail;
    std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> cp, cp0;
    if (!FullBundleAdjustmentSolver::ComputeCovarianceBatch(ptrs, sigma, &cp, nullptr, nullptr, &rels)) ++fail;
    if (!FullBundleAdjustmentSolver::ComputeCovarianceBatch(ptrs, sigma, &cp0, nullptr)) ++fail;
    if (!fail && !(cp[0][3](0, 0) > 0.0 && cp[0][3](0, 0) < cp0[0][3](0, 0))) ++fail;  // information was added
    if (!FullBundleAdjustmentSolver::MarginalizeBatch(ptrs, marked, sigma, &marg, nullptr, &rels)) ++fail;
    if (!FullBundleAdjustmentSolver::MarginalizeBatch(ptrs, marked, sigma, &marg0)) ++fail;
    for (size_t k = 0; k < base.size() && !fail; ++k)
      if (!LeftAsExpected(base[k], rels[k], marg[k]) || marg[k].dim != marg0[k].dim || marg[k].H == marg0[k].H ||
          !marg0[k].relatives_left.empty())
        ++fail;
    // malformed input throws: a list too few, an unknown pointer, two fixed poses, j == k
    std::vector<std::vector<Rel>> bad = rels;
    bad.pop_back();
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(ptrs, options, nullptr, nullptr, sigma, &bad); })) ++fail;
    bad = rels;
    _BA_Pose stranger = _BA_Pose::Identity();
    bad[1][0].pose_j = &stranger;
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(ptrs, options, nullptr, nullptr, sigma, &bad); })) ++fail;
    bad = rels;
    bad[0][0].pose_j = &base[0].poses[0];  // (0, 1): both fixed, refused by the library before the GPU is touched
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(ptrs, options, nullptr, nullptr, sigma, &bad); })) ++fail;
    bad = rels;
    bad[0][1].pose_k = bad[0][1].pose_j;
    if (!Throws([&] { FullBundleAdjustmentSolver::SolveBatch(ptrs, options, nullptr, nullptr, sigma, &bad); })) ++fail;
  }
  std::vector<std::vector<Rel>> stayed;
  if (!fail) {
    std::vector<std::unique_ptr<FullBundleAdjustmentSolver>> own;
    std::vector<FullBundleAdjustmentSolver *> ptrs;
    std::vector<InPrior> in;
    for (size_t k = 0; k < base.size(); ++k) {
      own.emplace_back(new FullBundleAdjustmentSolver());
      FullBundleAdjustmentSolver &s = *own.back();
      s.SetVerbose(false);
      for (size_t c = 0; c < base[k].cams.size(); ++c) s.AddCamera(static_cast<int>(c), base[k].cams[c]);
      RegisterReduced(s, base[k], marg[k], [&](_BA_Pose *p) { s.AddPose(p); }, [&](_BA_Point *q) { s.AddPoint(q); });
      ptrs.push_back(&s);
      in.emplace_back(marg[k]);
      stayed.push_back(Stayed(rels[k], marg[k]));
    }
    const std::vector<Window> before = base;
    if (!FullBundleAdjustmentSolver::SolveBatch(ptrs, options, nullptr, &in, sigma, &stayed)) ++fail;
    double moved = 0.0;
    for (size_t k = 0; k < base.size(); ++k)
      for (size_t j = 2; j < base[k].poses.size(); ++j)
        if (static_cast<int>(j) != kMarked)
          moved = std::max(moved, (base[k].poses[j].translation() - before[k].poses[j].translation()).norm());
    std::printf("reduced windows with the prior and %zu + %zu factors that stayed: largest move %.3e\n",
                stayed[0].size(), stayed[1].size(), moved);
    if (!(moved > 0.0 && std::isfinite(moved))) ++fail;
  }
  // ---- FullBundleAdjustmentSolverRefactor: the same chain, the same bits ---------------------
  if (!fail) {
    std::vector<Window> win = start;
    std::vector<std::vector<Rel>> rr;
    for (Window &w : win) rr.push_back(MakeFactors(w, sigma));
    std::vector<Prior> m;
    {
      std::vector<std::unique_ptr<FullBundleAdjustmentSolverRefactor>> own;
      std::vector<FullBundleAdjustmentSolverRefactor *> ptrs;
      std::vector<std::vector<_BA_Pose *>> marked;
      for (size_t k = 0; k < win.size(); ++k) {
        own.emplace_back(new FullBundleAdjustmentSolverRefactor());
        FullBundleAdjustmentSolverRefactor &r = *own.back();
        RegisterRefactor(r, win[k]);
        for (auto &T : win[k].poses) r.RegisterWorldToBodyPose(&T);
        for (auto &X : win[k].points) r.RegisterWorldPoint(&X);
        for (size_t j = 0; j < win[k].poses.size(); ++j)
          if (win[k].fixed_pose[j]) r.MakePoseFixed(&win[k].poses[j]);
        for (const auto &o : win[k].obs) r.AddObservation(o.c, &win[k].poses[o.j], &win[k].points[o.i], o.uv);
        ptrs.push_back(&r);
        marked.push_back({&win[k].poses[kMarked]});
      }
      if (!FullBundleAdjustmentSolverRefactor::SolveBatch(ptrs, options, nullptr, nullptr, sigma, &rr)) ++fail;
      std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> cp;
      if (!FullBundleAdjustmentSolverRefactor::ComputeCovarianceBatch(ptrs, sigma, &cp, nullptr, nullptr, &rr)) ++fail;
      if (!FullBundleAdjustmentSolverRefactor::MarginalizeBatch(ptrs, marked, sigma, &m, nullptr, &rr)) ++fail;
      for (size_t k = 0; k < win.size() && !fail; ++k)
        if (m[k].H != marg[k].H || m[k].b != marg[k].b || m[k].relatives_left != marg[k].relatives_left) ++fail;
    }
    if (!fail) {
      std::vector<std::unique_ptr<FullBundleAdjustmentSolverRefactor>> own;
      std::vector<FullBundleAdjustmentSolverRefactor *> ptrs;
      std::vector<InPrior> in;
      std::vector<std::vector<Rel>> st;
      for (size_t k = 0; k < win.size(); ++k) {
        own.emplace_back(new FullBundleAdjustmentSolverRefactor());
        FullBundleAdjustmentSolverRefactor &r = *own.back();
        RegisterRefactor(r, win[k]);
        RegisterReduced(r, win[k], m[k], [&](_BA_Pose *p) { r.RegisterWorldToBodyPose(p); },
                        [&](_BA_Point *q) { r.RegisterWorldPoint(q); });
        ptrs.push_back(&r);
        in.emplace_back(m[k]);
        st.push_back(Stayed(rr[k], m[k]));
      }
      if (!FullBundleAdjustmentSolverRefactor::SolveBatch(ptrs, options, nullptr, &in, sigma, &st)) ++fail;
      double diff = 0.0;
      for (size_t k = 0; k < win.size(); ++k) {
        for (size_t j = 0; j < win[k].poses.size(); ++j)
          for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c)
              diff = std::max(diff, std::fabs(win[k].poses[j].linear()(r, c) - base[k].poses[j].linear()(r, c)));
            diff = std::max(diff, std::fabs(win[k].poses[j].translation()(r) - base[k].poses[j].translation()(r)));
          }
        for (size_t i = 0; i < win[k].points.size(); ++i)
          for (int r = 0; r < 3; ++r) diff = std::max(diff, std::fabs(win[k].points[i](r) - base[k].points[i](r)));
      }
      std::printf("refactored class against the first, after the whole chain: %.2e\n", diff);
      if (diff != 0.0) ++fail;
    }
  }
  std::printf(fail ? "BATCH RELATIVE FACADE TEST FAILED (%d)\n" : "BATCH RELATIVE FACADE TEST PASSED\n", fail);
  return fail ? 1 : 0;
}
