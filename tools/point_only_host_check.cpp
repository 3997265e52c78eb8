// Stand-alone host check of ba_point_only's validation, packing and unpacking
// (bundle_adjustment_solver_amd/csrc/ba_point_only_host.h), meant for the host sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude tools/point_only_host_check.cpp -o /tmp/point_only_host_check && /tmp/point_only_host_check
// No GPU and no HIP: the device's part of a call is played by copying the uploaded points
// into place and filling results and rows with a pattern.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../bundle_adjustment_solver_amd/csrc/ba_point_only_host.h"

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                     \
    }                                                               \
  } while (0)

static int one_case(const std::vector<int> &counts, int cap, bool with_tri) {
  const int n_pt = (int)counts.size(), n_cam = 2, n_pose = 3;
  std::vector<int64_t> off(n_pt + 1, 0);
  for (int i = 0; i < n_pt; ++i) off[i + 1] = off[i] + counts[i];
  const int64_t n_obs = off[n_pt];
  // exactly-sized arrays (one entry where there is no observation: the pointers may not be
  // NULL): an access past an end is the sanitizer's to find
  const size_t n_arr = n_obs ? (size_t)n_obs : 1;
  std::vector<int32_t> cam(n_arr), pose(n_arr);
  std::vector<double> uv(n_arr * 2), X((size_t)n_pt * 3), intr(n_cam * 4, 1.0), Tc(n_cam * 12, 0.5),
      Tp(n_pose * 12, 0.25);
  std::vector<uint8_t> tri((size_t)n_pt);
  for (int64_t k = 0; k < n_obs; ++k) {
    cam[k] = (int32_t)(k % n_cam);
    pose[k] = (int32_t)(k % n_pose);
    uv[2 * k] = 0.1 * (double)k;
    uv[2 * k + 1] = -0.2 * (double)k;
  }
  for (int i = 0; i < n_pt; ++i) {
    tri[i] = (uint8_t)(i % 2);
    for (int c = 0; c < 3; ++c) X[3 * i + c] = i + 0.25 * c;
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (n_pt > 2) X[3 * 2 + 1] = nan;   // landmark 2: status 1 unless triangulated / empty
  Tp[12 * 2 + 5] = nan;               // pose 2: whoever observes through it is status 1
  std::string err;
  REQUIRE(ba::point_only_validate(n_cam, n_pose, n_pt, off.data(), cam.data(), pose.data(), &err) == 0);
  ba::PointOnlyBlob B;
  ba::point_only_pack(n_cam, intr.data(), Tc.data(), n_pose, Tp.data(), n_pt, off.data(), cam.data(), pose.data(),
                      uv.data(), with_tri ? tri.data() : nullptr, X.data(), cap, &B);
  REQUIRE(B.h2d_end <= B.end && B.host.size() == B.end && B.X < B.h2d_end);
  const uint8_t *flag = B.host.data() + B.flag;
  for (int i = 0; i < n_pt; ++i) {
    const bool t = with_tri && tri[i];
    REQUIRE(((flag[i] & 4) != 0) == t);
    bool uses_pose2 = false;
    for (int64_t k = off[i]; k < off[i + 1]; ++k) uses_pose2 |= pose[k] == 2;
    const int want = counts[i] == 0 ? 2 : ((uses_pose2 || (i == 2 && !t)) ? 1 : 0);
    REQUIRE((flag[i] & 3) == want);
  }
  // the device's part: results and rows
  ba_point_result *dr = (ba_point_result *)(B.host.data() + B.res);
  ba_iter_info *drow = (ba_iter_info *)(B.host.data() + B.rows);
  for (int i = 0; i < n_pt; ++i) {
    dr[i].n_rows = cap ? (i % (cap + 1)) : 0;
    dr[i].status = flag[i] & 3;
    for (int k = 0; k < dr[i].n_rows; ++k) drow[(size_t)i * cap + k].cost = 100.0 * i + k;
  }
  std::vector<double> Xo((size_t)n_pt * 3);
  std::vector<ba_point_result> res((size_t)n_pt);
  std::vector<ba_iter_info> rows((size_t)n_pt * cap);
  ba::point_only_unpack(B, n_pt, Xo.data(), cap ? rows.data() : nullptr, cap, res.data());
  for (int i = 0; i < n_pt; ++i) {
    REQUIRE(std::memcmp(&Xo[3 * i], &X[3 * i], 3 * sizeof(double)) == 0);
    for (int k = 0; k < res[i].n_rows; ++k) REQUIRE(rows[(size_t)i * cap + k].cost == 100.0 * i + k);
  }
  return 0;
}

int main() {
  const std::vector<std::vector<int>> cases = {{5}, {0}, {1}, {2, 0, 3}, {0, 0, 0}, {16, 17, 33, 1, 0, 8}, {0, 4}, {4, 0}};
  for (const auto &c : cases)
    for (int cap : {0, 1, 7})
      for (bool t : {false, true})
        if (one_case(c, cap, t)) return 1;
  // refusals: the message names the landmark / observation
  std::string err;
  const int64_t off[4] = {0, 2, 2, 5}, dec[4] = {0, 2, 1, 5}, first[4] = {1, 2, 2, 5};
  int32_t cam[5] = {0, 1, 0, 1, 0}, pose[5] = {0, 1, 2, 0, 1};
  REQUIRE(ba::point_only_validate(2, 3, 3, off, cam, pose, &err) == 0);
  REQUIRE(ba::point_only_validate(2, 3, 3, dec, cam, pose, &err) == -1 && err.find("landmark 1") != err.npos);
  REQUIRE(ba::point_only_validate(2, 3, 3, first, cam, pose, &err) == -1);
  REQUIRE(ba::point_only_validate(2, 3, 0, off, cam, pose, &err) == -1);
  REQUIRE(ba::point_only_validate(2, 3, 3, nullptr, cam, pose, &err) == -1);
  REQUIRE(ba::point_only_validate(2, 3, 3, off, nullptr, pose, &err) == -1);
  cam[3] = 2;
  REQUIRE(ba::point_only_validate(2, 3, 3, off, cam, pose, &err) == -1 &&
          err.find("observation 3 (landmark 2)") != err.npos);
  cam[3] = 1;
  pose[4] = -1;
  REQUIRE(ba::point_only_validate(2, 3, 3, off, cam, pose, &err) == -1 &&
          err.find("observation 4 (landmark 2)") != err.npos);
  std::printf("POINT ONLY HOST CHECK PASSED\n");
  return 0;
}
