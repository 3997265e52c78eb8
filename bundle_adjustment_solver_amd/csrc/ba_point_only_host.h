// ba_point_only_host.h — host side of ba_point_only (ba_point_only.hip): validation of the
// structure, packing of the caller's arrays into the one buffer a call uploads, and the
// way back.  Plain C++ with no HIP call, so that it also builds into a stand-alone
// program under the host sanitizers (tools/point_only_host_check.cpp).  Internal.
#ifndef BA_POINT_ONLY_HOST_H_
#define BA_POINT_ONLY_HOST_H_

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ba_hip.h"

namespace ba {

// Everything ba_point_only_check refuses; *err names the landmark / observation.
inline int point_only_validate(int n_cam, int n_pose, int n_pt, const int64_t *obs_off, const int32_t *obs_cam,
                               const int32_t *obs_pose, std::string *err) {
  auto bad = [&](const std::string &m) {
    *err = m;
    return -1;
  };
  if (n_cam < 1) return bad("n_cam must be >= 1");
  if (n_pose < 1) return bad("n_pose must be >= 1");
  if (n_pt < 1) return bad("n_pt must be >= 1");
  if (!obs_off) return bad("null obs_off");
  if (!obs_cam || !obs_pose) return bad("null obs_cam / obs_pose");
  if (obs_off[0] != 0) return bad("obs_off[0] must be 0");
  for (int i = 0; i < n_pt; ++i)
    if (obs_off[i + 1] < obs_off[i]) return bad("obs_off decreases at landmark " + std::to_string(i));
  int i = 0;
  for (int64_t k = 0; k < obs_off[n_pt]; ++k) {
    while (obs_off[i + 1] <= k) ++i;
    if (obs_cam[k] < 0 || obs_cam[k] >= n_cam)
      return bad("camera index " + std::to_string(obs_cam[k]) + " out of range at observation " +
                 std::to_string(k) + " (landmark " + std::to_string(i) + ")");
    if (obs_pose[k] < 0 || obs_pose[k] >= n_pose)
      return bad("pose index " + std::to_string(obs_pose[k]) + " out of range at observation " +
                 std::to_string(k) + " (landmark " + std::to_string(i) + ")");
  }
  return 0;
}

// The buffer of one call.  [0, h2d_end) goes up; [X, end) comes back: the points, the
// results and the iteration rows.
struct PointOnlyBlob {
  std::vector<uint8_t> host;
  size_t cams = 0, poses = 0, off = 0, uv = 0, cp = 0, flag = 0, X = 0, res = 0, rows = 0, h2d_end = 0, end = 0;
};

inline bool point_only_finite(const double *p, int n) {
  double s = 0.0;
  for (int k = 0; k < n; ++k) s += p[k] * 0.0;  // NaN or Inf anywhere -> NaN
  return s == 0.0;
}

// flag[i]: bits 0..1 = the status the host can decide (2: no observations; 1: a non-finite
// value among the landmark's inputs — its X unless triangulated, its pixels, cameras,
// poses; no observations wins over non-finite), bit 2 = triangulate.  The structure has
// passed point_only_validate.
inline void point_only_pack(int n_cam, const double *intr4, const double *T_cj12, int n_pose, const double *T_jw12,
                            int n_pt, const int64_t *obs_off, const int32_t *obs_cam, const int32_t *obs_pose,
                            const double *obs_uv2, const uint8_t *triangulate, const double *X3, int cap,
                            PointOnlyBlob *B) {
  const int64_t n_obs = obs_off[n_pt];
  size_t at = 0;
  auto take = [&](size_t bytes) {
    const size_t o = at;
    at += (bytes + 15) & ~(size_t)15;
    return o;
  };
  B->cams = take((size_t)n_cam * 16 * sizeof(double));
  B->poses = take((size_t)n_pose * 12 * sizeof(double));
  B->off = take((size_t)(n_pt + 1) * sizeof(int64_t));
  B->uv = take((size_t)n_obs * 2 * sizeof(double));
  B->cp = take((size_t)n_obs * 2 * sizeof(int32_t));
  B->flag = take((size_t)n_pt);
  B->X = take((size_t)n_pt * 3 * sizeof(double));
  B->h2d_end = at;
  B->res = take((size_t)n_pt * sizeof(ba_point_result));
  B->rows = take((size_t)n_pt * (size_t)cap * sizeof(ba_iter_info));
  B->end = at;
  B->host.assign(B->end, 0);
  uint8_t *hb = B->host.data();
  std::vector<uint8_t> cam_bad((size_t)n_cam), pose_bad((size_t)n_pose);
  double *cams = (double *)(hb + B->cams);
  for (int c = 0; c < n_cam; ++c) {
    std::memcpy(cams + (size_t)c * 16, intr4 + (size_t)c * 4, 4 * sizeof(double));
    std::memcpy(cams + (size_t)c * 16 + 4, T_cj12 + (size_t)c * 12, 12 * sizeof(double));
    cam_bad[c] = !point_only_finite(cams + (size_t)c * 16, 16);
  }
  std::memcpy(hb + B->poses, T_jw12, (size_t)n_pose * 12 * sizeof(double));
  for (int p = 0; p < n_pose; ++p) pose_bad[p] = !point_only_finite(T_jw12 + (size_t)p * 12, 12);
  std::memcpy(hb + B->off, obs_off, (size_t)(n_pt + 1) * sizeof(int64_t));
  if (n_obs > 0) std::memcpy(hb + B->uv, obs_uv2, (size_t)n_obs * 2 * sizeof(double));
  int32_t *cp = (int32_t *)(hb + B->cp);
  uint8_t *flag = hb + B->flag;
  for (int i = 0; i < n_pt; ++i) {
    const bool tri = triangulate && triangulate[i];
    bool bad = !tri && !point_only_finite(X3 + (size_t)i * 3, 3);
    for (int64_t k = obs_off[i]; k < obs_off[i + 1]; ++k) {
      cp[2 * k] = obs_cam[k];
      cp[2 * k + 1] = obs_pose[k];
      bad = bad || cam_bad[obs_cam[k]] || pose_bad[obs_pose[k]] || !point_only_finite(obs_uv2 + 2 * k, 2);
    }
    const int st = obs_off[i + 1] == obs_off[i] ? 2 : (bad ? 1 : 0);
    flag[i] = (uint8_t)(st | (tri ? 4 : 0));
  }
  std::memcpy(hb + B->X, X3, (size_t)n_pt * 3 * sizeof(double));
}

// After the download: points, results, and the rows each landmark wrote.
inline void point_only_unpack(const PointOnlyBlob &B, int n_pt, double *X3, ba_iter_info *rows, int cap,
                              ba_point_result *res) {
  const uint8_t *hb = B.host.data();
  std::memcpy(X3, hb + B.X, (size_t)n_pt * 3 * sizeof(double));
  std::memcpy(res, hb + B.res, (size_t)n_pt * sizeof(ba_point_result));
  if (!rows || cap <= 0) return;
  const ba_iter_info *hr = (const ba_iter_info *)(hb + B.rows);
  for (int i = 0; i < n_pt; ++i) {
    int nr = res[i].n_rows;
    if (nr > cap) nr = cap;
    if (nr > 0) std::memcpy(rows + (size_t)i * cap, hr + (size_t)i * cap, (size_t)nr * sizeof(ba_iter_info));
  }
}

}  // namespace ba
#endif  // BA_POINT_ONLY_HOST_H_
