// PoseOnlyBundleAdjustmentSolver — C++ facade of the pose-only path over the
// HIP C ABI.  Mirrors all four entry points of the reference
// (core/pose_only_bundle_adjustment_solver.h:25-67): monocular and stereo, planar
// 3-DoF and 6-DoF, with the reference's signatures.
#ifndef BA_FACADE_POSE_ONLY_BUNDLE_ADJUSTMENT_SOLVER_H_
#define BA_FACADE_POSE_ONLY_BUNDLE_ADJUSTMENT_SOLVER_H_

#include <vector>

#include "core/solver_option_and_summary.h"
#include "eigen3/Eigen/Dense"
#include "eigen3/Eigen/Geometry"

struct ba_handle;

namespace visual_navigation {
namespace analytic_solver {

class PoseOnlyBundleAdjustmentSolver {
 public:
  PoseOnlyBundleAdjustmentSolver();
  ~PoseOnlyBundleAdjustmentSolver();
  PoseOnlyBundleAdjustmentSolver(const PoseOnlyBundleAdjustmentSolver &) = delete;

  // reference core/pose_only_bundle_adjustment_solver.h:28-48, .cpp:401-615 / :617-900
  bool Solve_Monocular_Planar3Dof(const std::vector<Eigen::Vector3f> &world_position_list,
                                  const std::vector<Eigen::Vector2f> &matched_pixel_list, const float fx,
                                  const float fy, const float cx, const float cy,
                                  const Eigen::Isometry3f &pose_base_to_camera,
                                  const Eigen::Isometry3f &pose_world_to_last,
                                  Eigen::Isometry3f &pose_world_to_current, std::vector<bool> &mask_inlier,
                                  Options options, Summary *summary = nullptr);
  bool Solve_Stereo_Planar3Dof(const std::vector<Eigen::Vector3f> &world_position_list,
                               const std::vector<Eigen::Vector2f> &matched_left_pixel_list,
                               const std::vector<Eigen::Vector2f> &matched_right_pixel_list, const float fx_left,
                               const float fy_left, const float cx_left, const float cy_left, const float fx_right,
                               const float fy_right, const float cx_right, const float cy_right,
                               const Eigen::Isometry3f &base_to_camera_pose,
                               const Eigen::Isometry3f &left_to_right_pose,
                               const Eigen::Isometry3f &world_to_last_pose, Eigen::Isometry3f &world_to_current_pose,
                               std::vector<bool> &mask_inlier_left, std::vector<bool> &mask_inlier_right,
                               Options options, Summary *summary = nullptr);

  bool Solve_Monocular_6Dof(const std::vector<Eigen::Vector3f> &reference_position_list,
                            const std::vector<Eigen::Vector2f> &matched_pixel_list, const float fx, const float fy,
                            const float cx, const float cy, Eigen::Isometry3f &reference_to_current_pose,
                            std::vector<bool> &mask_inlier, Options options, Summary *summary = nullptr);

  // reference core/pose_only_bundle_adjustment_solver.h (Solve_Stereo_6Dof), .cpp:172-399
  bool Solve_Stereo_6Dof(const std::vector<Eigen::Vector3f> &reference_position_list,
                         const std::vector<Eigen::Vector2f> &matched_left_pixel_list,
                         const std::vector<Eigen::Vector2f> &matched_right_pixel_list, const float fx_left,
                         const float fy_left, const float cx_left, const float cy_left, const float fx_right,
                         const float fy_right, const float cx_right, const float cy_right,
                         const Eigen::Isometry3f &left_to_right_pose,
                         Eigen::Isometry3f &reference_to_current_left_pose, std::vector<bool> &mask_inlier_left,
                         std::vector<bool> &mask_inlier_right, Options options, Summary *summary = nullptr);

  // Many 6-DoF problems in one GPU launch (ba_pose_only_{mono,stereo}6_batch):
  // one frame = the arguments of one Solve_Monocular_6Dof / Solve_Stereo_6Dof
  // call, its in/out pose and masks, its Summary and its success flag, updated
  // as the single call updates them (a frame of <= 2048 points gets the single
  // call's bits).  Every size check comes before any device use.  Returns true
  // when every frame succeeded.  Frames without points are left as they are
  // (success).  GetDebugPoses() is empty afterwards.
  struct MonocularFrame6Dof {
    std::vector<Eigen::Vector3f> reference_position_list;
    std::vector<Eigen::Vector2f> matched_pixel_list;
    float fx{0.0f}, fy{0.0f}, cx{0.0f}, cy{0.0f};
    Eigen::Isometry3f reference_to_current_pose;
    std::vector<bool> mask_inlier;
    Summary summary;
    bool success{false};
  };
  struct StereoFrame6Dof {
    std::vector<Eigen::Vector3f> reference_position_list;
    std::vector<Eigen::Vector2f> matched_left_pixel_list;
    std::vector<Eigen::Vector2f> matched_right_pixel_list;
    float fx_left{0.0f}, fy_left{0.0f}, cx_left{0.0f}, cy_left{0.0f};
    float fx_right{0.0f}, fy_right{0.0f}, cx_right{0.0f}, cy_right{0.0f};
    Eigen::Isometry3f left_to_right_pose;
    Eigen::Isometry3f reference_to_current_left_pose;
    std::vector<bool> mask_inlier_left, mask_inlier_right;
    Summary summary;
    bool success{false};
  };
  bool Solve_Monocular_6Dof_Batch(std::vector<MonocularFrame6Dof> &frames, Options options);
  bool Solve_Stereo_6Dof_Batch(std::vector<StereoFrame6Dof> &frames, Options options);

  // Many planar 3-DoF problems in one GPU launch (ba_pose_only_{mono,stereo}3_batch),
  // as the 6-DoF batch above: one frame = the arguments of one
  // Solve_Monocular_Planar3Dof / Solve_Stereo_Planar3Dof call, its in/out pose
  // (world_to_current) and masks, its Summary and its success flag.  A frame
  // without points is left as it is (success), where the single planar call
  // returns true without solving too.
  struct MonocularFramePlanar3Dof {
    std::vector<Eigen::Vector3f> world_position_list;
    std::vector<Eigen::Vector2f> matched_pixel_list;
    float fx{0.0f}, fy{0.0f}, cx{0.0f}, cy{0.0f};
    Eigen::Isometry3f pose_base_to_camera;
    Eigen::Isometry3f pose_world_to_last;
    Eigen::Isometry3f pose_world_to_current;
    std::vector<bool> mask_inlier;
    Summary summary;
    bool success{false};
  };
  struct StereoFramePlanar3Dof {
    std::vector<Eigen::Vector3f> world_position_list;
    std::vector<Eigen::Vector2f> matched_left_pixel_list;
    std::vector<Eigen::Vector2f> matched_right_pixel_list;
    float fx_left{0.0f}, fy_left{0.0f}, cx_left{0.0f}, cy_left{0.0f};
    float fx_right{0.0f}, fy_right{0.0f}, cx_right{0.0f}, cy_right{0.0f};
    Eigen::Isometry3f base_to_camera_pose;
    Eigen::Isometry3f left_to_right_pose;
    Eigen::Isometry3f world_to_last_pose;
    Eigen::Isometry3f world_to_current_pose;
    std::vector<bool> mask_inlier_left, mask_inlier_right;
    Summary summary;
    bool success{false};
  };
  bool Solve_Monocular_Planar3Dof_Batch(std::vector<MonocularFramePlanar3Dof> &frames, Options options);
  bool Solve_Stereo_Planar3Dof_Batch(std::vector<StereoFramePlanar3Dof> &frames, Options options);

  const std::vector<Eigen::Isometry3f> &GetDebugPoses() const;

 private:
  // one frame's Summary after a batched call (Row = ba_po_iter, Result =
  // ba_po_result of include/ba_hip.h; defined in the .cpp)
  template <class Row, class Result>
  static void FillBatchSummary(const Options &options, Summary &summary, const Row *rows, int cap,
                               const Result &r, double ms);

  ba_handle *handle_{nullptr};
  std::vector<Eigen::Isometry3f> debug_poses_;
};

}  // namespace analytic_solver
}  // namespace visual_navigation
#endif
