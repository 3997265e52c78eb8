// GPU test of the pose graph's covariance and gate on the C++ facades
// (ComputePoseGraphCovariance, GateLoopClosures; ba_pgraph_covariance and ba_pgraph_gate of
// include/ba_hip.h).  A chain of 12 poses (pose 0 fixed) with drifted start values carries an
// odometry chain and three loop closures.  Both classes must return what the C calls give on the
// same arrays in scaled units (the facade's preprocessing restated here), converted by the unit
// relations of the header: Sigma_user = unit^2 D Sigma_scaled D with unit = sigma_pixel * 0.01 and
// D = diag(100 I, I), d2_user = d2_scaled / unit^2, to 1e-12 relative.  A true candidate passes
// the 0.999 quantile of chi-square with 6 degrees of freedom, one that is 2 units off does not.
// Neither call moves a pose.  Then the refusals: factors or candidates with two values of
// sigma_pixel, a candidate that carries a robust kernel, no factor at all.
// Exit code 0 = pass.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ba_hip.h"
#include "core/full_bundle_adjustment_solver.h"
#include "core/full_bundle_adjustment_solver_refactor.h"
#include "eigen3/Eigen/Dense"

using namespace visual_navigation::analytic_solver;
using Rel = FullBundleAdjustmentSolver::RelativePose;
using Mat6 = Eigen::Matrix<double, 6, 6>;
constexpr int kPoses = 12;
constexpr double kGate = 22.46;  // chi-square, 6 degrees of freedom, 0.999

struct Graph {
  std::vector<_BA_Pose> poses, truth;
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
    g.poses[j].translation() += _BA_Point(0.001 * j * U(gen), 0.001 * j * U(gen), 0.001 * j * U(gen));
  return g;
}

static Rel MakeFactor(Graph &g, int j, int k, double sigma, double off) {
  const double wgt = 1.0 / (sigma * sigma * 1e-4);
  Rel r;
  r.pose_j = &g.poses[j];
  r.pose_k = &g.poses[k];
  r.measurement = g.truth[j].inverse() * g.truth[k];
  r.measurement.translation() += _BA_Point(0.001 + off, -0.0005 - 0.5 * off, 0.0008);
  for (int a = 0; a < 6; ++a) {
    const double da = a < 3 ? 0.01 : 1.0;
    r.information[6 * a + a] = wgt * da * (a < 3 ? 2e4 : 2e2) * da;
  }
  r.information[6 * 4 + 1] = r.information[6 * 1 + 4] = wgt * 0.01 * 3e2;
  return r;
}

static std::vector<Rel> MakeFactors(Graph &g, double sigma) {
  std::vector<Rel> out;
  for (int q = 0; q + 1 < kPoses; ++q) out.push_back(MakeFactor(g, q + 1, q, sigma, 0.0));
  out.push_back(MakeFactor(g, kPoses - 1, 2, sigma, 0.0));
  out.push_back(MakeFactor(g, 3, 9, sigma, 0.0));
  out.push_back(MakeFactor(g, 0, 6, sigma, 0.0));  // j fixed
  return out;
}

// a true candidate, a false one (2 units off), one with the fixed pose
static std::vector<Rel> MakeCandidates(Graph &g, double sigma) {
  return {MakeFactor(g, 10, 4, sigma, 0.0), MakeFactor(g, 4, 10, sigma, 2.0), MakeFactor(g, 8, 0, sigma, 0.0)};
}

static void Pack(const _BA_Pose &P, std::vector<double> &v) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) v.push_back(P.linear()(r, c));
  for (int r = 0; r < 3; ++r) v.push_back(P.translation()(r));
}

#define TRY(expr)                                             \
  do {                                                        \
    if ((expr) != 0) {                                        \
      std::printf("%s failed: %s\n", #expr, ba_last_error()); \
      return false;                                           \
    }                                                         \
  } while (0)

struct Scaled {
  std::vector<int32_t> j, k;
  std::vector<double> Z, Om;
};
// the facade's preprocessing of factors restated
static Scaled Scale(const Graph &g, const std::vector<Rel> &rels, double sigma) {
  const double s = 0.01, inv = 100.0, wgt = 1.0 / (sigma * sigma * s * s);
  Scaled out;
  for (const Rel &r : rels) {
    out.j.push_back(static_cast<int32_t>(r.pose_j - &g.poses[0]));
    out.k.push_back(static_cast<int32_t>(r.pose_k - &g.poses[0]));
    _BA_Pose Zs = r.measurement;
    Zs.translation() = Zs.translation() * s;
    Pack(Zs, out.Z);
    for (int rr = 0; rr < 6; ++rr)
      for (int c = 0; c < 6; ++c)
        out.Om.push_back(((rr < 3 ? inv : 1.0) * r.information[6 * rr + c] * (c < 3 ? inv : 1.0)) / wgt);
  }
  return out;
}

struct DirectResult {
  std::vector<double> pose, cross, rel, d2;  // scaled units
};

static bool Direct(const Graph &g, const std::vector<Rel> &rels, const std::vector<Rel> &cands, double sigma,
                   const std::vector<int32_t> &sel, const std::vector<int32_t> &pj, const std::vector<int32_t> &pk,
                   DirectResult *out) {
  std::vector<double> Tp;
  std::vector<uint8_t> pf(g.poses.size(), 0);
  pf[0] = 1;
  for (const _BA_Pose &pose : g.poses) {
    _BA_Pose P = pose.inverse();
    P.translation() = P.translation() * 0.01;
    Pack(P, Tp);
  }
  const Scaled f = Scale(g, rels, sigma), c = Scale(g, cands, sigma);
  ba_handle *h = nullptr;
  TRY(ba_create(&h, 0));
  ba_pgraph *pg = nullptr;
  TRY(ba_pgraph_create(&pg, h, static_cast<int>(g.poses.size()), Tp.data(), pf.data(), static_cast<int64_t>(f.j.size()),
                       f.j.data(), f.k.data(), f.Z.data(), f.Om.data()));
  out->pose.assign(36 * sel.size(), 0.0);
  out->cross.assign(36 * pj.size(), 0.0);
  out->rel.assign(36 * pj.size(), 0.0);
  out->d2.assign(cands.size(), 0.0);
  int64_t dropped = -1;
  TRY(ba_pgraph_covariance(pg, static_cast<int>(sel.size()), sel.data(), out->pose.data(),
                           static_cast<int64_t>(pj.size()), pj.data(), pk.data(), out->cross.data(), out->rel.data(),
                           &dropped));
  if (dropped != 0) return false;
  TRY(ba_pgraph_gate(pg, static_cast<int64_t>(cands.size()), c.j.data(), c.k.data(), c.Z.data(), c.Om.data(),
                     out->d2.data(), nullptr, nullptr, &dropped));
  std::vector<double> T(Tp.size());
  TRY(ba_pgraph_get_poses(pg, T.data()));
  ba_pgraph_destroy(pg);
  ba_destroy(h);
  return dropped == 0 && std::memcmp(T.data(), Tp.data(), T.size() * sizeof(double)) == 0;
}

// |got - unit^2 D want D| <= 1e-12 max|.| per block
static bool SameBlocks(const std::vector<Mat6> &got, const std::vector<double> &scaled, double unit) {
  if (got.size() * 36 != scaled.size()) return false;
  for (size_t s = 0; s < got.size(); ++s) {
    double big = 0.0, err = 0.0;
    for (int r = 0; r < 6; ++r)
      for (int c = 0; c < 6; ++c) {
        const double want = unit * unit * ((r < 3 ? 100.0 : 1.0) * scaled[36 * s + 6 * r + c] * (c < 3 ? 100.0 : 1.0));
        big = std::max(big, std::fabs(want));
        err = std::max(err, std::fabs(got[s](r, c) - want));
      }
    if (!(err <= 1e-12 * big)) return false;
  }
  return true;
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
static int FacadeCase(const char *name, const Graph &start, double sigma, void (*add_pose)(Solver &, _BA_Pose *)) {
  int fail = 0;
  Graph g = start;
  const std::vector<Rel> rels = MakeFactors(g, sigma), cands = MakeCandidates(g, sigma);
  const std::vector<int32_t> sel = {11, 1, 5, 5, 7}, pj = {11, 1, 6, 0}, pk = {1, 11, 7, 3};
  DirectResult want;
  if (!Direct(g, rels, cands, sigma, sel, pj, pk, &want)) {
    std::printf("%s: the direct calls failed\n", name);
    return 1;
  }
  Solver s;
  s.SetVerbose(false);
  for (auto &T : g.poses) add_pose(s, &T);
  s.MakePoseFixed(&g.poses[0]);
  if (!Throws([&] { s.GateLoopClosures(cands, sigma, nullptr); }, "null output")) ++fail;
  std::vector<double> d2;
  if (!Throws([&] { s.GateLoopClosures(cands, sigma, &d2); }, "must be added first")) ++fail;
  for (const Rel &r : rels) s.AddRelativePose(r, sigma);
  std::vector<_BA_Pose *> poses;
  for (int32_t p : sel) poses.push_back(&g.poses[p]);
  std::vector<std::pair<_BA_Pose *, _BA_Pose *>> pairs;
  for (size_t p = 0; p < pj.size(); ++p) pairs.emplace_back(&g.poses[pj[p]], &g.poses[pk[p]]);
  const std::vector<_BA_Pose> before = g.poses;
  std::vector<Mat6> cp, cc, cr;
  if (!s.ComputePoseGraphCovariance(poses, pairs, &cp, &cc, &cr)) ++fail;
  if (!s.GateLoopClosures(cands, sigma, &d2)) ++fail;
  const double unit = sigma * 0.01;
  bool same = SameBlocks(cp, want.pose, unit) && SameBlocks(cc, want.cross, unit) && SameBlocks(cr, want.rel, unit) &&
              d2.size() == want.d2.size();
  for (size_t c = 0; same && c < d2.size(); ++c)
    same = std::fabs(d2[c] - want.d2[c] / (unit * unit)) <= 1e-12 * std::fabs(d2[c]);
  std::printf("%s: %s; d2 = %.3f (true), %.3e (false), %.3f (with the fixed pose)\n", name,
              same ? "the direct calls in the caller's units" : "DIFFERENT", d2[0], d2[1], d2[2]);
  if (!same) ++fail;
  if (!(d2[0] < kGate) || !(d2[1] > 1e3) || !(d2[2] < kGate)) ++fail;
  for (size_t p = 0; p < g.poses.size(); ++p)  // neither call moves a pose
    if (!(g.poses[p].matrix() == before[p].matrix())) ++fail;
  // a null cross output is allowed; the other blocks are the same
  std::vector<Mat6> cp2, cr2;
  if (!s.ComputePoseGraphCovariance(poses, pairs, &cp2, nullptr, &cr2)) ++fail;
  for (size_t k = 0; k < cr.size(); ++k)
    if (!(cr[k] == cr2[k])) ++fail;
  // refusals
  if (!Throws([&] { s.ComputePoseGraphCovariance(poses, pairs, nullptr, nullptr, &cr2); }, "null output")) ++fail;
  if (!Throws([&] { s.ComputePoseGraphCovariance({&g.poses[0]}, {}, &cp2, nullptr, nullptr); }, "is a fixed pose"))
    ++fail;
  if (!Throws([&] { s.GateLoopClosures(cands, 2.0 * sigma, &d2); }, "sigma_pixel = 0.7 and 1.4")) ++fail;
  Rel robust = cands[0];
  robust.robust_kind = 2;
  robust.robust_scale = 3.0;
  if (!Throws([&] { s.GateLoopClosures({robust}, sigma, &d2); }, "carries a robust kernel")) ++fail;
  s.AddRelativePose(MakeFactor(g, 9, 2, 0.5, 0.0), 0.5);
  if (!Throws([&] { s.ComputePoseGraphCovariance(poses, pairs, &cp, &cc, &cr); }, "sigma_pixel = 0.7 and 0.5")) ++fail;
  return fail;
}

int main() {
  const Graph start = MakeGraph(1);
  const double sigma = 0.7;
  int fail = 0;
  fail += FacadeCase<FullBundleAdjustmentSolver>("FullBundleAdjustmentSolver", start, sigma,
                                                 [](FullBundleAdjustmentSolver &s, _BA_Pose *T) { s.AddPose(T); });
  fail += FacadeCase<FullBundleAdjustmentSolverRefactor>(
      "FullBundleAdjustmentSolverRefactor", start, sigma,
      [](FullBundleAdjustmentSolverRefactor &s, _BA_Pose *T) { s.RegisterWorldToBodyPose(T); });
  if (fail) {
    std::printf("%d checks failed\n", fail);
    return 1;
  }
  std::printf("POSE GRAPH COVARIANCE FACADE TEST PASSED\n");
  return 0;
}
