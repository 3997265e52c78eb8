// ba_point_only.hip — point-only ("structure-only") solves: every pose fixed, every
// landmark its own 3x3 Levenberg-Marquardt problem, all of them in ONE launch
// (ba_point_only / ba_point_only_check of include/ba_hip.h).
//
// Work split: a TEAM of W lanes (W = 8 or 16, inside one DPP row) owns one landmark;
// the lane is the observation.  A lane reads its observation's pixel, camera and pose
// once and keeps them in registers; a landmark with more than W observations walks the
// rest in team-sized steps from memory.  The ten sums of a linearisation (C_i, b_i, the
// cost) are added inside the team by a fixed DPP butterfly that leaves EVERY lane of the
// team with the same bits, so the 3x3 inverse, the step, the model and the control step
// are evaluated by all lanes of the team on identical values — the issue slots a single
// lane would use, and no broadcast.  Only the team's first lane writes (rows, result,
// point).  No LDS, no atomics, no barrier: a team whose landmark has stopped idles until
// the wave's last team stops, and the loop is bounded by max_num_iterations.
//
// Arithmetic: project / weight_and_G / make_R / spd3_inverse / lm_control_step of
// ba_device_fn.h, called; nothing of the control step is restated here.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ba_hip.h"
#include "ba_device_fn.h"
#include "ba_handle.h"
#include "ba_point_only_host.h"

namespace ba {
namespace {

constexpr int kPtBlock = 256;

// a pivot of the triangulation's normal equations below this fraction of their largest
// diagonal entry is "degenerate" (status 3).  The equations square the conditioning of
// the rows, so 1e-12 is a parallax of about 1e-6 rad; an exactly rank-deficient system
// leaves a pivot of rounding size, ~1e-16 of the diagonal.
constexpr double kTriPivot = 1e-12;

struct PtArgs {
  const double *cams;      // n_cam * 16
  const double *poses;     // n_pose * 12
  const int64_t *obs_off;  // n_pt + 1
  const double2 *uv;       // n_obs
  const int2 *cp;          // n_obs {camera, pose}
  const uint8_t *flag;     // n_pt: bits 0..1 = status decided on the host (0, 1, 2), bit 2 = triangulate
  double *X;               // n_pt * 3, in / out
  ba_point_result *res;    // n_pt
  DevIterRec *rows;        // n_pt * cap, or null
  int n_pt, cap;
  double lambda0, huber, thr_step, thr_cost, dec_ratio, inc_ratio;
  int max_iter, gn;
};

// sum over the team: xor-1, xor-2, half-mirror (W = 8) and mirror (W = 16).  Every step
// adds the same two partial sums in both partners (a + b == b + a), so every lane of the
// team ends with the same bits, and they do not depend on where in the wave the team sits.
template <int W>
__device__ __forceinline__ double team_sum(double v) {
  v += dpp_f64<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_f64<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_f64<0x141>(v);  // row_half_mirror
  if (W == 16) v += dpp_f64<0x140>(v);  // row_mirror
  return v;
}

// one observation's terms of C_i (6), b_i (3) and the cost (reference :811-823, :381-433)
__device__ __forceinline__ void obs_terms(const double *__restrict__ cam, const double *__restrict__ T,
                                          const double u, const double v, const double X0, const double X1,
                                          const double X2, const double huber, double acc[10]) {
  ObsGeom g;
  project(cam, T, X0, X1, X2, u, v, g);
  double w, G[6], Rm[6];
  weight_and_G(cam, g, huber, w, G);
  make_R(G, T, Rm);
  const double wr0 = w * g.r0, wr1 = w * g.r1;
  acc[0] += w * (Rm[0] * Rm[0] + Rm[3] * Rm[3]);
  acc[1] += w * (Rm[0] * Rm[1] + Rm[3] * Rm[4]);
  acc[2] += w * (Rm[0] * Rm[2] + Rm[3] * Rm[5]);
  acc[3] += w * (Rm[1] * Rm[1] + Rm[4] * Rm[4]);
  acc[4] += w * (Rm[1] * Rm[2] + Rm[4] * Rm[5]);
  acc[5] += w * (Rm[2] * Rm[2] + Rm[5] * Rm[5]);
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[6 + c] -= Rm[c] * wr0 + Rm[3 + c] * wr1;
  acc[9] += sqrt(g.r0 * g.r0 + g.r1 * g.r1);
}

// the two rows of the linear triangulation of one observation: with (R, t) = T_cj o T_jw,
// (r1 - x r3) . X = -(t1 - x t3) and (r2 - y r3) . X = -(t2 - y t3); acc = upper triangle
// of the normal matrix (6) and its right-hand side (3)
__device__ __forceinline__ void tri_terms(const double *__restrict__ cam, const double *__restrict__ T,
                                          const double u, const double v, double acc[9]) {
  const double *Rc = cam + 4, *tc = cam + 13;
  double R[9], t[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      R[r * 3 + c] = Rc[r * 3 + 0] * T[0 * 3 + c] + Rc[r * 3 + 1] * T[1 * 3 + c] + Rc[r * 3 + 2] * T[2 * 3 + c];
    t[r] = (Rc[r * 3 + 0] * T[9] + Rc[r * 3 + 1] * T[10] + Rc[r * 3 + 2] * T[11]) + tc[r];
  }
  const double xh = (u - cam[2]) / cam[0], yh = (v - cam[3]) / cam[1];
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    const double s = row ? yh : xh;
    const double a0 = R[row * 3 + 0] - s * R[6], a1 = R[row * 3 + 1] - s * R[7], a2 = R[row * 3 + 2] - s * R[8];
    const double rhs = -(t[row] - s * t[2]);
    acc[0] += a0 * a0;
    acc[1] += a0 * a1;
    acc[2] += a0 * a2;
    acc[3] += a1 * a1;
    acc[4] += a1 * a2;
    acc[5] += a2 * a2;
    acc[6] += a0 * rhs;
    acc[7] += a1 * rhs;
    acc[8] += a2 * rhs;
  }
}

template <int W>
__global__ __launch_bounds__(kPtBlock) void k_point_only(const PtArgs a) {
  const int team = blockIdx.x * (kPtBlock / W) + threadIdx.x / W, lane = threadIdx.x & (W - 1);
  if (team >= a.n_pt) return;  // a whole team leaves: no DPP step crosses a team
  const int fl = a.flag[team];
  ba_point_result *res = a.res + team;
  if (fl & 3) {  // decided on the host: non-finite input (1) or no observations (2)
    if (lane == 0) {
      res->n_iter = 0;
      res->converged = 0;
      res->n_rows = 0;
      res->status = fl & 3;
      res->n_behind = 0;
      res->dropped_pivots = 0;
      res->cost0 = 0.0;
      res->cost = 0.0;
    }
    return;
  }
  const int64_t o0 = a.obs_off[team], o1 = a.obs_off[team + 1];
  const int n = (int)(o1 - o0);
  // the lane's own observation, read once (lanes past the end keep harmless values and
  // are left out of every sum)
  const bool has = lane < n;
  double cam[16], T[12], u = 0.0, v = 0.0;
  {
    const int64_t k = has ? o0 + lane : o0;  // n >= 1 here
    const int2 ix = a.cp[k];
    const double2 p = a.uv[k];
    u = p.x;
    v = p.y;
#pragma unroll
    for (int e = 0; e < 16; ++e) cam[e] = a.cams[(size_t)ix.x * 16 + e];
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = a.poses[(size_t)ix.y * 12 + e];
  }
  double X0 = a.X[(size_t)team * 3 + 0], X1 = a.X[(size_t)team * 3 + 1], X2 = a.X[(size_t)team * 3 + 2];
  int status = 0;
  // ---- linear triangulation -------------------------------------------------------------
  if (fl & 4) {
    double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (has) tri_terms(cam, T, u, v, acc);
    for (int64_t k = o0 + lane + W; k < o1; k += W) {
      const int2 ix = a.cp[k];
      const double2 p = a.uv[k];
      tri_terms(a.cams + (size_t)ix.x * 16, a.poses + (size_t)ix.y * 12, p.x, p.y, acc);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) acc[e] = team_sum<W>(acc[e]);
    // LDL^T in the given order; every pivot against kTriPivot of the largest diagonal entry
    const double thr = kTriPivot * fmax(acc[0], fmax(acc[3], acc[5]));
    const double d0 = acc[0];
    const double l10 = acc[1] / d0, l20 = acc[2] / d0;
    const double d1 = acc[3] - l10 * acc[1];
    const double t21 = acc[4] - l20 * acc[1];
    const double l21 = t21 / d1;
    const double d2 = acc[5] - l20 * acc[2] - l21 * t21;
    if (n < 2 || !(thr > 0.0) || !(d0 > thr && d1 > thr && d2 > thr)) {
      status = 3;
    } else {
      const double z0 = acc[6], z1 = acc[7] - l10 * z0, z2 = acc[8] - l20 * z0 - l21 * z1;
      X2 = z2 / d2;
      X1 = z1 / d1 - l21 * X2;
      X0 = z0 / d0 - l10 * X1 - l20 * X2;
      if (!(isfinite(X0) && isfinite(X1) && isfinite(X2))) {
        status = 3;
        X0 = a.X[(size_t)team * 3 + 0];
        X1 = a.X[(size_t)team * 3 + 1];
        X2 = a.X[(size_t)team * 3 + 2];
      }
    }
  }
  // C_i, b_i and the cost at (x0, x1, x2), in every lane of the team
  auto linearize = [&](const double x0, const double x1, const double x2, double acc[10]) {
#pragma unroll
    for (int e = 0; e < 10; ++e) acc[e] = 0.0;
    if (has) obs_terms(cam, T, u, v, x0, x1, x2, a.huber, acc);
    for (int64_t k = o0 + lane + W; k < o1; k += W) {
      const int2 ix = a.cp[k];
      const double2 p = a.uv[k];
      obs_terms(a.cams + (size_t)ix.x * 16, a.poses + (size_t)ix.y * 12, p.x, p.y, x0, x1, x2, a.huber, acc);
    }
#pragma unroll
    for (int e = 0; e < 10; ++e) acc[e] = team_sum<W>(acc[e]);
  };
  DevCtrl c;
  c.iter = 0;
  c.converged = 0;
  double cost0 = 0.0, cost = 0.0;
  int dropped = 0;
  if (status == 0) {
    double L[10];  // the linearisation at the accepted point
    linearize(X0, X1, X2, L);
    cost0 = cost = L[9];
    c.lambda = a.lambda0;
    c.prev_cost = cost0;
    c.huber = a.huber;
    c.thr_step = a.thr_step;
    c.thr_cost = a.thr_cost;
    c.dec_ratio = a.dec_ratio;
    c.inc_ratio = a.inc_ratio;
    c.t_last = wall_clock64();
    c.cur = 0;
    c.lcur = 0;
    c.tcur = c.tlcur = 0;
    c.done = a.max_iter <= 0 ? 1 : 0;
    c.converged = a.max_iter <= 0 ? 1 : 0;
    c.max_iter = a.max_iter;
    c.gn = a.gn;
    DevIterRec *log = a.rows ? a.rows + (size_t)team * a.cap : nullptr;
    const int log_cap = (lane == 0 && a.rows) ? a.cap : 0;  // one writer per row
    while (!c.done) {
      // damp and invert (reference :846-856), step, model on the damped block (:435-455)
      const double lp1 = 1.0 + c.lambda;
      double cd[6] = {L[0] * lp1, L[1], L[2], L[3] * lp1, L[4], L[5] * lp1}, ci[6];
      spd3_inverse(cd, ci);
      if (!(ci[0] > 0.0 && ci[3] > 0.0 && ci[5] > 0.0)) ++dropped;
      const double b0 = L[6], b1 = L[7], b2 = L[8];
      const double y0 = ci[0] * b0 + ci[1] * b1 + ci[2] * b2;
      const double y1 = ci[1] * b0 + ci[3] * b1 + ci[4] * b2;
      const double y2 = ci[2] * b0 + ci[4] * b1 + ci[5] * b2;
      const double r0 = y0 * cd[0] + y1 * cd[1] + y2 * cd[2];
      const double r1 = y0 * cd[1] + y1 * cd[3] + y2 * cd[4];
      const double r2 = y0 * cd[2] + y1 * cd[4] + y2 * cd[5];
      const double est = (b0 * y0 + b1 * y1 + b2 * y2) + (r0 * y0 + r1 * y1 + r2 * y2);
      const double sy = sqrt(y0 * y0 + y1 * y1 + y2 * y2);
      // trial point: its cost, and the linearisation the next iteration needs if it is accepted
      const double t0 = X0 + y0, t1 = X1 + y1, t2 = X2 + y2;
      double Lt[10];
      linearize(t0, t1, t2, Lt);
      const int before = c.cur;
      lm_control_step(&c, log, log_cap, (double)n, 1, Lt[9], est, sy, 0.0);
      if (c.cur != before) {  // accepted
        X0 = t0;
        X1 = t1;
        X2 = t2;
        cost = Lt[9];
#pragma unroll
        for (int e = 0; e < 10; ++e) L[e] = Lt[e];
      }
    }
  }
  // observations behind their camera at the returned point
  double behind = 0.0;
  {
    ObsGeom g;
    if (has) {
      project(cam, T, X0, X1, X2, u, v, g);
      behind += (g.Xc[2] <= 0.0) ? 1.0 : 0.0;
    }
    for (int64_t k = o0 + lane + W; k < o1; k += W) {
      const int2 ix = a.cp[k];
      const double2 p = a.uv[k];
      project(a.cams + (size_t)ix.x * 16, a.poses + (size_t)ix.y * 12, X0, X1, X2, p.x, p.y, g);
      behind += (g.Xc[2] <= 0.0) ? 1.0 : 0.0;
    }
    behind = team_sum<W>(behind);
  }
  if (lane == 0) {
    if (status == 0) {
      a.X[(size_t)team * 3 + 0] = X0;
      a.X[(size_t)team * 3 + 1] = X1;
      a.X[(size_t)team * 3 + 2] = X2;
    }
    res->n_iter = c.iter;
    res->converged = c.converged;
    res->n_rows = a.rows ? min(c.iter, a.cap) : 0;
    res->status = status;
    res->n_behind = (int)behind;
    res->dropped_pivots = dropped;
    res->cost0 = cost0;
    res->cost = cost;
  }
}

thread_local double g_point_ms = 0.0;  // device time of this thread's last launch
int g_team_width = 8;                   // process-wide; see ba_point_only_team (8 measured faster)

}  // namespace
}  // namespace ba

// ---- C ABI.  The host side of a call — validation, packing, unpacking — is in
// ba_point_only_host.h (no HIP call; also built stand-alone for the host sanitizers).

extern "C" {

int ba_point_only_check(int n_cam, int n_pose, int n_pt, const int64_t *obs_off, const int32_t *obs_cam,
                        const int32_t *obs_pose) {
  std::string err;
  if (ba::point_only_validate(n_cam, n_pose, n_pt, obs_off, obs_cam, obs_pose, &err))
    return ba::fail("ba_point_only_check: " + err);
  return 0;
}

int ba_point_only_team(int width) {
  if (width == 0) return ba::g_team_width;
  if (width != 8 && width != 16) return ba::fail("ba_point_only_team: the width is 8 or 16 (0 asks)");
  ba::g_team_width = width;
  return width;
}

int ba_point_only_last_ms(double *kernel_ms) {
  if (!kernel_ms) return ba::fail("ba_point_only_last_ms: null pointer");
  *kernel_ms = ba::g_point_ms;
  return 0;
}

int ba_point_only(ba_handle *h, int n_cam, const double *intr4, const double *T_cj12, int n_pose,
                  const double *T_jw12, int n_pt, const int64_t *obs_off, const int32_t *obs_cam,
                  const int32_t *obs_pose, const double *obs_uv2, const uint8_t *triangulate, double *X3,
                  const ba_options *opt, ba_iter_info *rows, int cap, ba_point_result *res) {
  const std::string fn = "ba_point_only: ";
  if (!intr4 || !T_cj12 || !T_jw12 || !obs_uv2 || !X3 || !opt || !res) return ba::fail(fn + "null pointer");
  if (cap < 0) return ba::fail(fn + "cap must be >= 0");
  std::string err;
  if (ba::point_only_validate(n_cam, n_pose, n_pt, obs_off, obs_cam, obs_pose, &err)) return ba::fail(fn + err);
  if (!h) return ba::fail(fn + "null handle");  // (last: everything above is checked without a GPU)
  static_assert(sizeof(ba::DevIterRec) == sizeof(ba_iter_info), "iteration row layout");
  static_assert(sizeof(ba_point_result) == 40, "point result layout");
  const bool want_rows = rows && cap > 0;
  ba::PointOnlyBlob B;
  ba::point_only_pack(n_cam, intr4, T_cj12, n_pose, T_jw12, n_pt, obs_off, obs_cam, obs_pose, obs_uv2, triangulate,
                      X3, want_rows ? cap : 0, &B);
  // ---- one upload, one launch, one download, one synchronisation ------------------------
  HIP_TRY(hipSetDevice(h->device));
  ba::ScratchAllocs scratch(h);
  uint8_t *dev = nullptr;
  if (h->dalloc(ba::Mem::Resident, &dev, B.end)) return -1;
  hipStream_t s = h->stream;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_TRY(hipEventCreate(&e0));
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return ba::fail(fn + "hipEventCreate failed");
  }
  struct Events {
    hipEvent_t a, b;
    ~Events() {
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
    }
  } events{e0, e1};
  HIP_TRY(hipMemcpyAsync(dev, B.host.data(), B.h2d_end, hipMemcpyHostToDevice, s));
  ba::PtArgs a;
  a.cams = (const double *)(dev + B.cams);
  a.poses = (const double *)(dev + B.poses);
  a.obs_off = (const int64_t *)(dev + B.off);
  a.uv = (const double2 *)(dev + B.uv);
  a.cp = (const int2 *)(dev + B.cp);
  a.flag = dev + B.flag;
  a.X = (double *)(dev + B.X);
  a.res = (ba_point_result *)(dev + B.res);
  a.rows = want_rows ? (ba::DevIterRec *)(dev + B.rows) : nullptr;
  a.n_pt = n_pt;
  a.cap = want_rows ? cap : 0;
  a.lambda0 = (double)opt->initial_lambda;
  a.huber = (double)opt->threshold_huber_loss;
  a.thr_step = (double)opt->threshold_step_size;
  a.thr_cost = (double)opt->threshold_cost_change;
  a.dec_ratio = (double)opt->decrease_ratio_lambda;
  a.inc_ratio = (double)opt->increase_ratio_lambda;
  a.max_iter = opt->max_num_iterations;
  a.gn = opt->gauss_newton ? 1 : 0;
  const int width = ba::g_team_width;
  const int64_t lanes = (int64_t)n_pt * width;
  const unsigned grid = (unsigned)((lanes + ba::kPtBlock - 1) / ba::kPtBlock);
  HIP_TRY(hipEventRecord(e0, s));
  if (width == 8)
    hipLaunchKernelGGL(ba::k_point_only<8>, dim3(grid), dim3(ba::kPtBlock), 0, s, a);
  else
    hipLaunchKernelGGL(ba::k_point_only<16>, dim3(grid), dim3(ba::kPtBlock), 0, s, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(e1, s));
  HIP_TRY(hipMemcpyAsync(B.host.data() + B.X, dev + B.X, B.end - B.X, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
  ba::g_point_ms = (double)ms;
  ba::point_only_unpack(B, n_pt, X3, rows, want_rows ? cap : 0, res);
  return 0;
}

}  // extern "C"
