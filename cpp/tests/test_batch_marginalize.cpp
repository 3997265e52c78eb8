// GPU test of FullBundleAdjustmentSolver::MarginalizeBatch: two small windows (stereo 5
// poses, mono 6 poses; poses 0 and 1 fixed) whose oldest optimisable pose, which sees the
// first 18 landmarks only, is marked.  The priors from ONE MarginalizeBatch must equal
// ba_batch_marginalize called directly on the same arrays (the facade's preprocessing
// restated here: T_jw = inverse(pose), lengths and pixels scaled by 0.01) after the unit
// conversion H = D^-1 H_s D^-1 / (1e-4 sigma^2), b = D^-1 b_s / (1e-4 sigma^2), bit for
// bit: the two paths run the same kernel on the same numbers.  The kept poses and the
// marginalised points come back as the caller's pointers, an unknown pointer and a sharded
// solver throw, the refactored class forwards the call.  Exit code 0 = pass.
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

// ba_batch_marginalize on the arrays of the windows, converted to the caller's units
static bool Direct(std::vector<Window> &win, double sigma, std::vector<Prior> *out) {
  const double s = 0.01;
  std::vector<int32_t> cam_off{0}, pose_off{0}, pt_off{0}, oc, op, oq;
  std::vector<int64_t> obs_off{0};
  std::vector<double> intr, T_cj, T, X, uv;
  std::vector<uint8_t> pose_fixed, point_fixed, mark;
  auto pack = [](const _BA_Pose &P, std::vector<double> &v) {
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) v.push_back(P.linear()(r, c));
    for (int r = 0; r < 3; ++r) v.push_back(P.translation()(r));
  };
  for (Window &w : win) {
    for (const _BA_Camera &cam : w.cams) {
      intr.insert(intr.end(), {cam.fx * s, cam.fy * s, cam.cx * s, cam.cy * s});
      _BA_Pose P = cam.pose_this_to_cam0;
      P.translation() *= s;
      pack(P, T_cj);
    }
    for (size_t j = 0; j < w.poses.size(); ++j) {
      _BA_Pose P = w.poses[j].inverse();
      P.translation() = P.translation() * s;
      pack(P, T);
      pose_fixed.push_back(static_cast<uint8_t>(w.fixed_pose[j]));
      mark.push_back(static_cast<int>(j) == kMarked);
    }
    for (const _BA_Point &Q : w.points) {
      const _BA_Point Qs = Q * s;
      for (int r = 0; r < 3; ++r) X.push_back(Qs(r));
      point_fixed.push_back(0);
    }
    for (const auto &o : w.obs) {
      oc.push_back(o.c);
      op.push_back(o.j);
      oq.push_back(o.i);
      uv.push_back(o.uv(0) * s);
      uv.push_back(o.uv(1) * s);
    }
    cam_off.push_back(static_cast<int32_t>(intr.size() / 4));
    pose_off.push_back(static_cast<int32_t>(pose_fixed.size()));
    pt_off.push_back(static_cast<int32_t>(point_fixed.size()));
    obs_off.push_back(static_cast<int64_t>(oc.size()));
  }
  const int B = static_cast<int>(win.size());
  ba_handle *h = nullptr;
  ba_batch *batch = nullptr;
  std::vector<int64_t> H_off(B + 1), b_off(B + 1);
  std::vector<ba_batch_marg_result> res(B);
  std::vector<double> H, bv;
  int rc = ba_create(&h, 0);
  if (rc == 0)
    rc = ba_batch_create(&batch, h, B, cam_off.data(), pose_off.data(), pt_off.data(), obs_off.data(), intr.data(),
                         T_cj.data(), T.data(), pose_fixed.data(), X.data(), point_fixed.data(), oc.data(), op.data(),
                         oq.data(), uv.data());
  if (rc == 0) rc = ba_batch_marg_layout(batch, mark.data(), H_off.data(), b_off.data());
  if (rc == 0) {
    H.resize(H_off[B]);
    bv.resize(b_off[B]);
    rc = ba_batch_marginalize(batch, 1.0, mark.data(), H.data(), bv.data(), nullptr, res.data());
  }
  if (rc) std::printf("direct call failed: %s\n", ba_last_error());
  ba_batch_destroy(batch);
  ba_destroy(h);
  if (rc) return false;
  out->assign(B, Prior());
  const double wgt = 1.0 / (sigma * sigma * s * s);
  for (int b = 0; b < B; ++b) {
    Prior &p = (*out)[b];
    p.dim = static_cast<int>(b_off[b + 1] - b_off[b]);
    p.status = res[b].status;
    p.dropped_pivots = res[b].dropped_pivots;
    p.H.resize(static_cast<size_t>(p.dim) * p.dim);
    p.b.resize(p.dim);
    for (int r = 0; r < p.dim; ++r) {
      const double dr = r % 6 < 3 ? s : 1.0;
      for (int c = 0; c < p.dim; ++c)
        p.H[static_cast<size_t>(r) * p.dim + c] =
            wgt * (dr * H[H_off[b] + static_cast<size_t>(r) * p.dim + c] * (c % 6 < 3 ? s : 1.0));
      p.b[r] = wgt * (dr * bv[b_off[b] + r]);
    }
  }
  return true;
}

int main() {
  std::vector<Window> win = {MakeWindow(5, 30, true, 1), MakeWindow(6, 26, false, 2)};
  const double sigma = 0.7;
  std::vector<std::unique_ptr<FullBundleAdjustmentSolver>> own;
  std::vector<FullBundleAdjustmentSolver *> ptrs;
  std::vector<std::vector<_BA_Pose *>> marked;
  for (size_t k = 0; k < win.size(); ++k) {
    own.emplace_back(new FullBundleAdjustmentSolver());
    Register(*own.back(), win[k]);
    ptrs.push_back(own.back().get());
    marked.push_back({&win[k].poses[kMarked]});
  }
  std::vector<Prior> got, want;
  int fail = FullBundleAdjustmentSolver::MarginalizeBatch(ptrs, marked, sigma, &got) ? 0 : 1;
  if (!Direct(win, sigma, &want)) ++fail;
  if (got.size() != win.size() || want.size() != win.size()) ++fail;
  for (size_t k = 0; k < win.size() && !fail; ++k) {
    Window &w = win[k];
    const Prior &g = got[k], &d = want[k];
    const int K = static_cast<int>(w.poses.size()) - 3;
    if (g.dim != 6 * K || d.dim != g.dim || g.status != 0 || g.dropped_pivots != 0) {
      ++fail;
      break;
    }
    double scale = 0.0, diff = 0.0, asym = 0.0, bmax = 0.0;
    for (int r = 0; r < g.dim; ++r) {
      for (int c = 0; c < g.dim; ++c) {
        scale = std::max(scale, std::fabs(d(r, c)));
        diff = std::max(diff, std::fabs(g(r, c) - d(r, c)));
        asym = std::max(asym, std::fabs(g(r, c) - g(c, r)));
      }
      diff = std::max(diff, std::fabs(g.b[r] - d.b[r]));
      bmax = std::max(bmax, std::fabs(g.b[r]));
    }
    std::printf("window %zu: K = %d, max |H| %.3e, max |b| %.3e, facade vs direct call %.2e, asymmetry %.2e\n", k, K,
                scale, bmax, diff, asym);
    if (!(scale > 0.0 && bmax > 0.0 && diff == 0.0 && asym == 0.0)) ++fail;
    // the kept poses and the marginalised points, as the caller's pointers
    if (g.kept_poses.size() != static_cast<size_t>(K) || g.marginalized_points.size() != static_cast<size_t>(kSeen)) {
      ++fail;
      break;
    }
    for (int t = 0; t < K; ++t)
      if (g.kept_poses[t] != &w.poses[3 + t]) ++fail;
    for (int i = 0; i < kSeen; ++i)
      if (g.marginalized_points[i] != &w.points[i]) ++fail;
  }
  // an unknown pointer, a wrong number of lists, a sharded solver
  {
    _BA_Pose stranger = _BA_Pose::Identity();
    std::vector<Prior> tmp;
    if (!Throws([&] { FullBundleAdjustmentSolver::MarginalizeBatch(ptrs, {{&stranger}, {}}, sigma, &tmp); })) ++fail;
    if (!Throws([&] { FullBundleAdjustmentSolver::MarginalizeBatch(ptrs, {{}}, sigma, &tmp); })) ++fail;
    Window w = win[0];
    FullBundleAdjustmentSolver sharded;
    Register(sharded, w);
    sharded.SetShard(0, 2);
    std::vector<FullBundleAdjustmentSolver *> mix = {ptrs[0], &sharded};
    if (!Throws([&] { FullBundleAdjustmentSolver::MarginalizeBatch(mix, {{}, {}}, sigma, &tmp); })) ++fail;
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
    std::vector<Prior> rp;
    if (!FullBundleAdjustmentSolverRefactor::MarginalizeBatch({&r}, {{&w.poses[kMarked]}}, sigma, &rp)) ++fail;
    if (rp.size() != 1 || got.size() != 2 || rp[0].dim != got[1].dim) {
      ++fail;
    } else {
      if (rp[0].H != got[1].H || rp[0].b != got[1].b) ++fail;
      if (rp[0].kept_poses.empty() || rp[0].kept_poses[0] != &w.poses[3]) ++fail;
    }
  }
  std::printf(fail ? "BATCH MARGINALIZE FACADE TEST FAILED (%d)\n" : "BATCH MARGINALIZE FACADE TEST PASSED\n", fail);
  return fail ? 1 : 0;
}
