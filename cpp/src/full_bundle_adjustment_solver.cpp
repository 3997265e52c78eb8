// Host facade of the full BA solver: see the header.  Reference line numbers
// refer to core/full_bundle_adjustment_solver.cpp.
#include "core/full_bundle_adjustment_solver.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <sstream>
#include <stdexcept>

#include "ba_hip.h"
#include "core/graph_session.h"

namespace visual_navigation {
namespace analytic_solver {

namespace {
void Pack12(const _BA_Pose &T, double *out) {  // row-major R, then t
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) out[3 * r + c] = T.linear()(r, c);
  for (int r = 0; r < 3; ++r) out[9 + r] = T.translation()(r);
}
_BA_Pose Unpack12(const double *in) {
  _BA_Pose T;
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) T.linear()(r, c) = in[3 * r + c];
    T.translation()(r) = in[9 + r];
  }
  return T;
}
void Check(int rc, const char *what) {
  if (rc < 0) throw std::runtime_error(std::string(what) + ": " + ba_last_error());
}
}  // namespace

FullBundleAdjustmentSolver::FullBundleAdjustmentSolver() {
  if (verbose_) std::cout << "SparseBundleAdjustmentSolver() - initialize.\n";  // :41
}

FullBundleAdjustmentSolver::~FullBundleAdjustmentSolver() {
  if (handle_) ba_destroy(handle_);
}

void FullBundleAdjustmentSolver::Reset() {  // :44-70
  if (handle_) ba_destroy(handle_);
  handle_ = nullptr;
  owned_points_.clear();
  is_parameter_finalized_ = false;
  camera_ids_.clear();
  cameras_.clear();
  pose_index_.clear();
  poses_.clear();
  T_jw_.clear();
  fixed_poses_.clear();
  point_index_.clear();
  points_.clear();
  X_.clear();
  fixed_points_.clear();
  observations_.clear();
  relatives_ = GraphFactors();
  sim3_ = GraphFactors();
  num_fixed_poses_ = num_fixed_points_ = 0;
}

void FullBundleAdjustmentSolver::AddCamera(const _BA_Index camera_index, const _BA_Camera &camera) {  // :72-85
  if (std::find(camera_ids_.begin(), camera_ids_.end(), camera_index) != camera_ids_.end())
    return;  // unordered_map::insert keeps the first
  _BA_Camera scaled = camera;
  scaled.pose_this_to_cam0.translation() *= scaler_;
  scaled.fx *= scaler_;
  scaled.fy *= scaler_;
  scaled.cx *= scaler_;
  scaled.cy *= scaler_;
  camera_ids_.push_back(camera_index);
  cameras_.push_back(scaled);
  if (verbose_)
    std::cout << "New camera is added.\n  fx: " << scaled.fx << ", fy: " << scaled.fy << ", cx: " << scaled.cx
              << ", cy: " << scaled.cy << "\n";
}

void FullBundleAdjustmentSolver::AddPose(_BA_Pose *original_pose) {  // :87-101
  if (is_parameter_finalized_) {
    std::cerr << TEXT_YELLOW("Cannot enroll parameter. (is_parameter_finalized_ == true)") << std::endl;
    return;
  }
  if (pose_index_.count(original_pose)) return;
  _BA_Pose T_jw = original_pose->inverse();
  T_jw.translation() = T_jw.translation() * scaler_;
  pose_index_[original_pose] = static_cast<int>(poses_.size());
  poses_.push_back(original_pose);
  T_jw_.push_back(T_jw);
}

void FullBundleAdjustmentSolver::AddRelativePose(const RelativePose &factor, double sigma_pixel) {
  if (is_parameter_finalized_) {
    std::cerr << TEXT_YELLOW("Cannot enroll parameter. (is_parameter_finalized_ == true)") << std::endl;
    return;
  }
  const std::vector<std::vector<RelativePose>> one(1, std::vector<RelativePose>(1, factor));
  RelativeArrays a;
  PackRelatives({this}, "AddRelativePose", &one, sigma_pixel, &a);
  relatives_.j.push_back(a.j[0]);
  relatives_.k.push_back(a.k[0]);
  relatives_.Z.insert(relatives_.Z.end(), a.Z.begin(), a.Z.begin() + 12);
  relatives_.Omega.insert(relatives_.Omega.end(), a.Omega.begin(), a.Omega.begin() + 36);
  relatives_.kind.push_back(a.kind[0]);
  relatives_.scale.push_back(a.scale[0]);
  relatives_.unit.push_back(a.unit[0]);
}

void FullBundleAdjustmentSolver::AddPoint(_BA_Point *original_point) {  // :103-117
  if (is_parameter_finalized_) {
    std::cerr << TEXT_YELLOW("Cannot enroll parameter. (is_parameter_finalized_ == true)\n");
    return;
  }
  if (point_index_.count(original_point)) return;
  point_index_[original_point] = static_cast<int>(points_.size());
  points_.push_back(original_point);
  X_.push_back((*original_point) * scaler_);
}

void FullBundleAdjustmentSolver::MakePoseFixed(_BA_Pose *original_poseptr) {  // :119-134
  if (is_parameter_finalized_) {
    std::cerr << TEXT_YELLOW("Cannot enroll parameter. (is_parameter_finalized_ == true)\n");
    return;
  }
  if (original_poseptr == nullptr) {
    std::cerr << "Empty pointer is conveyed. Skip this one.\n";
    return;
  }
  auto it = pose_index_.find(original_poseptr);
  if (it == pose_index_.end()) throw std::runtime_error("There is no pointer in the BA pose pool.");
  fixed_poses_.insert(it->second);
  ++num_fixed_poses_;
}

void FullBundleAdjustmentSolver::MakePointFixed(_BA_Point *original_pointptr_to_be_fixed) {  // :136-153
  if (is_parameter_finalized_) {
    std::cerr << TEXT_YELLOW("Cannot enroll parameter. (is_parameter_finalized_ == true)\n");
    return;
  }
  if (original_pointptr_to_be_fixed == nullptr) {
    std::cerr << "Empty pointer is conveyed. Skip this one.\n";
    return;
  }
  auto it = point_index_.find(original_pointptr_to_be_fixed);
  if (it == point_index_.end()) throw std::runtime_error("There is no pointer in the BA point pool.");
  fixed_points_.insert(it->second);
  ++num_fixed_points_;
}

void FullBundleAdjustmentSolver::AddObservation(const _BA_Index camera_index, _BA_Pose *related_pose,
                                                _BA_Point *related_point, const _BA_Pixel &pixel) {  // :155-180
  const auto cam_it = std::find(camera_ids_.begin(), camera_ids_.end(), camera_index);
  if (cam_it == camera_ids_.end()) {
    std::cerr << TEXT_RED("Invalid camera index.\n");
    return;
  }
  const auto pose_it = pose_index_.find(related_pose);
  if (pose_it == pose_index_.end()) {
    std::cerr << TEXT_RED("Nonexisting pose.\n");
    return;
  }
  const auto point_it = point_index_.find(related_point);
  if (point_it == point_index_.end()) {
    std::cerr << TEXT_RED("Nonexisting point.\n");
    return;
  }
  Observation o;
  o.camera_index = static_cast<int>(cam_it - camera_ids_.begin());
  o.pose_index = pose_it->second;
  o.point_index = point_it->second;
  o.u = pixel(0) * scaler_;
  o.v = pixel(1) * scaler_;
  observations_.push_back(o);
}

void FullBundleAdjustmentSolver::FinalizeParameters() {  // :182-206, :243-308, :668-700
  if (is_parameter_finalized_) return;
  for (size_t f = 0; f < relatives_.kind.size(); ++f)
    if (relatives_.kind[f] != 0)
      throw std::runtime_error("FinalizeParameters: factor " + std::to_string(f) +
                               " carries a robust kernel; robust factors are pose-graph only (SolvePoseGraph)");
  if (cameras_.empty() || poses_.empty() || points_.empty())
    throw std::runtime_error("FinalizeParameters: cameras, poses and points must be added first");
  Check(ba_create(&handle_, device_id_), "ba_create");
  std::vector<double> intr, T_cj(12 * cameras_.size());
  for (size_t c = 0; c < cameras_.size(); ++c) {
    intr.insert(intr.end(), {cameras_[c].fx, cameras_[c].fy, cameras_[c].cx, cameras_[c].cy});
    Pack12(cameras_[c].pose_this_to_cam0, &T_cj[12 * c]);
  }
  Check(ba_set_cameras(handle_, static_cast<int>(cameras_.size()), intr.data(), T_cj.data()), "ba_set_cameras");
  std::vector<double> T(12 * poses_.size()), X(3 * points_.size());
  std::vector<uint8_t> pose_fixed(poses_.size(), 0), point_fixed(points_.size(), 0);
  for (size_t p = 0; p < poses_.size(); ++p) {
    Pack12(T_jw_[p], &T[12 * p]);
    pose_fixed[p] = fixed_poses_.count(static_cast<int>(p)) > 0;
  }
  for (size_t q = 0; q < points_.size(); ++q) {
    for (int r = 0; r < 3; ++r) X[3 * q + r] = X_[q](r);
    point_fixed[q] = fixed_points_.count(static_cast<int>(q)) > 0;
  }
  Check(ba_set_poses(handle_, static_cast<int>(poses_.size()), T.data(), pose_fixed.data()), "ba_set_poses");
  Check(ba_set_points(handle_, static_cast<int>(points_.size()), X.data(), point_fixed.data()), "ba_set_points");
  std::vector<int32_t> oc(observations_.size()), op(observations_.size()), oq(observations_.size());
  std::vector<double> uv(2 * observations_.size());
  for (size_t k = 0; k < observations_.size(); ++k) {  // insertion order matters (:826)
    oc[k] = observations_[k].camera_index;
    op[k] = observations_[k].pose_index;
    oq[k] = observations_[k].point_index;
    uv[2 * k] = observations_[k].u;
    uv[2 * k + 1] = observations_[k].v;
  }
  Check(ba_set_observations(handle_, static_cast<int64_t>(oc.size()), oc.data(), op.data(), oq.data(), uv.data()),
        "ba_set_observations");
  if (shard_world_ > 1) Check(ba_set_shard(handle_, shard_rank_, shard_world_), "ba_set_shard");
  if (!relatives_.j.empty())
    Check(ba_set_relative(handle_, static_cast<int64_t>(relatives_.j.size()), relatives_.j.data(), relatives_.k.data(),
                          relatives_.Z.data(), relatives_.Omega.data()),
          "ba_set_relative");
  Check(ba_finalize(handle_), "ba_finalize");
  if (allreduce_fn_) Check(ba_set_allreduce(handle_, allreduce_fn_, allreduce_user_), "ba_set_allreduce");
  is_parameter_finalized_ = true;
}

void FullBundleAdjustmentSolver::ReloadParameterValues() {
  if (!is_parameter_finalized_) {  // nothing planned yet: refresh the copies FinalizeParameters will read
    for (size_t p = 0; p < poses_.size(); ++p) {
      T_jw_[p] = poses_[p]->inverse();
      T_jw_[p].translation() = T_jw_[p].translation() * scaler_;
    }
    for (size_t q = 0; q < points_.size(); ++q) X_[q] = (*points_[q]) * scaler_;
    return;
  }
  std::vector<double> T(12 * poses_.size()), X(3 * points_.size());
  for (size_t p = 0; p < poses_.size(); ++p) {
    T_jw_[p] = poses_[p]->inverse();
    T_jw_[p].translation() = T_jw_[p].translation() * scaler_;
    Pack12(T_jw_[p], &T[12 * p]);
  }
  for (size_t q = 0; q < points_.size(); ++q) {
    X_[q] = (*points_[q]) * scaler_;
    for (int r = 0; r < 3; ++r) X[3 * q + r] = X_[q](r);
  }
  Check(ba_update_values(handle_, T.data(), X.data()), "ba_update_values");
}

void FullBundleAdjustmentSolver::SetAllReduce(int (*fn)(void *, int, void *, int64_t, void *), void *user) {
  allreduce_fn_ = fn;
  allreduce_user_ = user;
  if (is_parameter_finalized_) Check(ba_set_allreduce(handle_, fn, user), "ba_set_allreduce");
}

bool FullBundleAdjustmentSolver::OwnsPoint(const _BA_Point *point) const {
  const auto it = point_index_.find(const_cast<_BA_Point *>(point));
  if (it == point_index_.end()) return false;
  return owned_points_.empty() || owned_points_[static_cast<size_t>(it->second)] != 0;
}

std::string FullBundleAdjustmentSolver::GetSolverStatistics() const {  // :208-239 (returns "")
  const size_t n_opt_pose = poses_.size() - fixed_poses_.size();
  const size_t n_opt_point = points_.size() - fixed_points_.size();
  std::cout << "| Bundle Adjustment Statistics:\n"
            << "| # cameras in rigid body system: " << cameras_.size() << "\n"
            << "|   " << TEXT_CYAN("(Note: The reference camera is 'camera_list_[0]'.)") << "\n"
            << "|             # of total poses: " << poses_.size() << "\n"
            << "|               - # fix  poses: " << num_fixed_poses_ << "\n"
            << "|               - # opt. poses: " << n_opt_pose << "\n"
            << "|            # of total points: " << points_.size() << "\n"
            << "|              - # fix  points: " << num_fixed_points_ << "\n"
            << "|              - # opt. points: " << n_opt_point << "\n"
            << "|            # of observations: " << observations_.size() << "\n"
            << "|                Jacobian size: " << 6 * observations_.size() << " rows x "
            << 3 * n_opt_point + 6 * n_opt_pose << " cols\n"
            << "|                Residual size: " << 2 * observations_.size() << " rows\n"
            << std::endl;
  return std::string();
}

void FullBundleAdjustmentSolver::CheckPoseAndPointConnectivity() {  // :310-341
  static constexpr int kMinNumObservedPoints = 5;
  static constexpr int kMinNumRelatedPoses = 2;
  // distinct related points per pose (only "fewer than 5" matters: the first
  // five distinct ids are kept) and distinct related poses per point (first id
  // + "a second one exists"); fixed partners count (:684-693)
  std::vector<std::array<int, kMinNumObservedPoints>> seen(poses_.size());
  std::vector<int> n_seen(poses_.size(), 0), first_pose(points_.size(), -1);
  std::vector<char> second_pose(points_.size(), 0);
  for (const Observation &o : observations_) {
    int &n = n_seen[o.pose_index];
    if (n < kMinNumObservedPoints) {
      auto &ids = seen[o.pose_index];
      if (std::find(ids.begin(), ids.begin() + n, o.point_index) == ids.begin() + n) ids[n++] = o.point_index;
    }
    if (first_pose[o.point_index] < 0)
      first_pose[o.point_index] = o.pose_index;
    else if (first_pose[o.point_index] != o.pose_index)
      second_pose[o.point_index] = 1;
  }
  // optimisation indices: input order of the non-fixed entries (the reference's
  // are unordered_map iteration order)
  int j_opt = 0;
  for (size_t p = 0; p < poses_.size(); ++p) {
    if (fixed_poses_.count(static_cast<int>(p))) continue;
    if (n_seen[p] < kMinNumObservedPoints)
      std::cerr << TEXT_YELLOW(std::to_string(j_opt) +
                               "-th pose: It might diverge because some frames "
                               "have insufficient related points.")
                << std::endl;
    ++j_opt;
  }
  int i_opt = 0;
  for (size_t q = 0; q < points_.size(); ++q) {
    if (fixed_points_.count(static_cast<int>(q))) continue;
    const int num_related_pose = (first_pose[q] >= 0 ? 1 : 0) + (second_pose[q] ? 1 : 0);
    if (num_related_pose < kMinNumRelatedPoses)
      std::cerr << TEXT_YELLOW(std::to_string(i_opt) +
                               "-th point: It might diverge because some "
                               "points have insufficient related poses.")
                << std::endl;
    ++i_opt;
  }
}

namespace {

ba_options PackOptions(const Options &options, bool gauss_newton) {
  ba_options o;
  o.threshold_step_size = options.convergence_handle.threshold_step_size;
  o.threshold_cost_change = options.convergence_handle.threshold_cost_change;
  o.threshold_huber_loss = options.outlier_handle.threshold_huber_loss;
  o.threshold_outlier_rejection = options.outlier_handle.threshold_outlier_rejection;
  o.max_num_iterations = options.iteration_handle.max_num_iterations;
  o.initial_lambda = options.trust_region_handle.initial_lambda;
  o.decrease_ratio_lambda = options.trust_region_handle.decrease_ratio_lambda;
  o.increase_ratio_lambda = options.trust_region_handle.increase_ratio_lambda;
  o.gauss_newton = gauss_newton ? 1 : 0;
  return o;
}

OptimizationInfo ToInfo(const ba_iter_info &row) {
  OptimizationInfo info;
  info.cost = row.cost;
  info.cost_change = row.cost_change;
  info.average_reprojection_error = row.average_reprojection_error;
  info.abs_step = row.abs_step;
  info.abs_gradient = 0;
  info.damping_term = row.damping_term;
  info.iter_time = row.iter_time_ms;
  info.iteration_status = static_cast<IterationStatus>(row.iteration_status);
  return info;
}

}  // namespace

void FullBundleAdjustmentSolver::BeginSummary(Summary *summary, const Options &options) {
  if (summary == nullptr) return;
  summary->max_iteration_ = options.iteration_handle.max_num_iterations;
  summary->threshold_cost_change_ = options.convergence_handle.threshold_cost_change;
  summary->threshold_step_size_ = options.convergence_handle.threshold_step_size;
  summary->convergence_status_ = true;
}

template <class Row>
void FullBundleAdjustmentSolver::FinishSummary(Summary *summary, const std::vector<Row> &rows, int n_iter, int converged,
                                               timer::StopWatch &stopwatch) {
  if (summary == nullptr) return;
  for (int k = 0; k < n_iter && k < static_cast<int>(rows.size()); ++k)
    summary->optimization_info_list_.push_back(ToInfo(rows[k]));
  summary->convergence_status_ = converged != 0;
  summary->total_time_in_millisecond_ = stopwatch.GetLapTimeFromStart();
}

void FullBundleAdjustmentSolver::WriteBack(const double *T_jw12, const double *X3, const uint8_t *valid) {
  for (size_t p = 0; p < poses_.size(); ++p) {
    if (fixed_poses_.count(static_cast<int>(p))) continue;
    _BA_Pose T_jw = Unpack12(&T_jw12[12 * p]);
    T_jw_[p] = T_jw;
    T_jw.translation() *= inverse_scaler_;
    *poses_[p] = T_jw.inverse();
  }
  for (size_t q = 0; q < points_.size(); ++q) {
    if (fixed_points_.count(static_cast<int>(q)) || !valid[q]) continue;
    X_[q] = _BA_Point(X3[3 * q], X3[3 * q + 1], X3[3 * q + 2]);
    *points_[q] = X_[q] * inverse_scaler_;
  }
}

bool FullBundleAdjustmentSolver::Solve(Options options, Summary *summary) {  // :630-1044
  return Run(options, summary, false);
}

// gradient_descent: FullBundleAdjustmentSolverRefactor::SolveByGradientDescent (reference
// core/full_bundle_adjustment_solver_refactor.cpp:1075-1367, ba_solve_gd) instead of the LM
// loop; the write-back and the Summary are the same
bool FullBundleAdjustmentSolver::Run(Options options, Summary *summary, bool gradient_descent) {
  timer::StopWatch stopwatch("BundleAdjustmentSolver::Solve");
  stopwatch.Start();
  BeginSummary(summary, options);
  FinalizeParameters();
  if (verbose_) GetSolverStatistics();
  CheckPoseAndPointConnectivity();  // :703

  const ba_options o = PackOptions(options, gauss_newton_);
  std::vector<ba_iter_info> rows(static_cast<size_t>(std::max(1, o.max_num_iterations)));
  int n_iter = 0, converged = 0;
  if (gradient_descent)
    Check(ba_solve_gd(handle_, &o, rows.data(), static_cast<int>(rows.size()), &n_iter, &converged), "ba_solve_gd");
  else
    Check(ba_solve(handle_, &o, rows.data(), static_cast<int>(rows.size()), &n_iter, &converged), "ba_solve");

  // write back through the caller's pointers (:1011-1022)
  std::vector<double> T(12 * poses_.size()), X(3 * points_.size());
  Check(ba_get_poses(handle_, T.data()), "ba_get_poses");
  // sharded: one final sum-all-reduce of the owned landmark rows, so that EVERY rank
  // writes back EVERY point, as the reference's contract says (:1018-1022)
  owned_points_.assign(points_.size(), 1);
  Check(ba_get_points(handle_, X.data(), owned_points_.data()), "ba_get_points");  // (+ which landmarks are this shard's)
  std::vector<uint8_t> valid(owned_points_);
  if (shard_world_ > 1 && allreduce_fn_) {
    Check(ba_gather_points(handle_), "ba_gather_points");
    Check(ba_get_points(handle_, X.data(), valid.data()), "ba_get_points");
  }
  WriteBack(T.data(), X.data(), valid.data());
  FinishSummary(summary, rows, n_iter, converged, stopwatch);
  return true;  // the reference always returns true (:1043)
}

// ---- the two pose graphs: one path at the width of Abi ----
namespace {

// The facade's counterpart of the library's GraphSpec: what a kind of graph is in the C ABI
// (include/ba_hip.h) and in the messages.  The handle entries are the same for both.
struct HandleAbi {
  using Handle = ba_handle;
  static constexpr const char *kCreateHandle = "ba_create";
  static constexpr auto create_handle = ba_create;
  static constexpr auto destroy_handle = ba_destroy;
  static constexpr auto last_error = ba_last_error;
};

struct Se3Abi : HandleAbi {
  using Graph = ba_pgraph;
  static constexpr int kWidth = 6, kPose = 12;  // tangent width, doubles per pose
  static constexpr const char *kPrefix = "ba_pgraph_", *kAdd = "AddRelativePose";
  static constexpr auto create = ba_pgraph_create;
  static constexpr auto set_robust = ba_pgraph_set_robust;
  static constexpr auto solve = ba_pgraph_solve;
  static constexpr auto get_poses = ba_pgraph_get_poses;
  static constexpr auto covariance = ba_pgraph_covariance;
  static constexpr auto gate = ba_pgraph_gate;
  static constexpr auto destroy = ba_pgraph_destroy;
  static void PackPose(const _BA_Pose &T, double *out) { Pack12(T, out); }
  // always s and w
  static int FactorReport(ba_pgraph *g, const std::vector<int32_t> &, double *s, std::vector<double> *w,
                          const char **entry) {
    *entry = "factor_report";
    return ba_pgraph_factor_report(g, s, w->data());
  }
};

struct Sim3Abi : HandleAbi {
  using Graph = ba_sim3;
  static constexpr int kWidth = 7, kPose = 13;
  static constexpr const char *kPrefix = "ba_sim3_", *kAdd = "AddRelativeSim3";
  static constexpr auto create = ba_sim3_create;
  static constexpr auto set_robust = ba_sim3_set_robust;
  static constexpr auto solve = ba_sim3_solve;
  static constexpr auto get_poses = ba_sim3_get_poses;
  static constexpr auto covariance = ba_sim3_covariance;
  static constexpr auto gate = ba_sim3_gate;
  static constexpr auto destroy = ba_sim3_destroy;
  static void PackPose(const _BA_Pose &T, double *out) {  // the similarity (R, t, s = 1)
    Pack12(T, out);
    out[12] = 1.0;
  }
  // s and w where a factor carries a kernel; no kernel: the report of before with w = 1, nothing
  // robust is allocated or launched
  static int FactorReport(ba_sim3 *g, const std::vector<int32_t> &kind, double *s, std::vector<double> *w,
                          const char **entry) {
    if (std::any_of(kind.begin(), kind.end(), [](int32_t kd) { return kd != 0; })) {
      *entry = "factor_weights";
      return ba_sim3_factor_weights(g, s, w->data());
    }
    *entry = "factor_report";
    w->assign(w->size(), 1.0);
    return ba_sim3_factor_report(g, s);
  }
};

// what Graph<Abi>::Run leaves: the poses as the graph got them and as it left them (Abi::kPose
// doubles each), and the rows of the solve
struct GraphRun {
  std::vector<double> start, solved;
  std::vector<ba_iter_info> rows;
  int n_iter{0}, converged{0};
};

}  // namespace

template <class Abi>
struct FullBundleAdjustmentSolver::Graph {
  using Solver = FullBundleAdjustmentSolver;
  using Block = Eigen::Matrix<double, Abi::kWidth, Abi::kWidth>;

  static void Require(const Solver &s, const char *who, const GraphFactors &f) {
    if (s.poses_.empty() || f.j.empty())
      throw std::runtime_error(std::string(who) + ": poses (AddPose) and factors (" + Abi::kAdd +
                               ") must be added first");
  }

  // the registered poses and the factors `f` as a graph with its kernels set, on the finalized
  // problem's handle or one of the session's own (the graph borrows it for its device and stream);
  // throws on a refusal.  *poses_out (may be null): the poses as the graph got them.
  static GraphSession<Abi> Open(const Solver &s, const char *who, const GraphFactors &f,
                                std::vector<double> *poses_out = nullptr) {
    Require(s, who, f);
    const size_t n_pose = s.poses_.size();
    std::vector<double> P(Abi::kPose * n_pose);
    std::vector<uint8_t> pose_fixed(n_pose, 0);
    for (size_t p = 0; p < n_pose; ++p) {
      Abi::PackPose(s.T_jw_[p], &P[Abi::kPose * p]);
      pose_fixed[p] = s.fixed_poses_.count(static_cast<int>(p)) > 0;
    }
    if (poses_out != nullptr) *poses_out = P;
    return GraphSession<Abi>(s.handle_, s.device_id_,
                             {static_cast<int>(n_pose), P.data(), pose_fixed.data(), static_cast<int64_t>(f.j.size()),
                              f.j.data(), f.k.data(), f.Z.data(), f.Omega.data(), f.kind.data(), f.scale.data()});
  }

  // the one unit sigma_pixel scaler_ of the factors and `more` (throws if there are two)
  static double Unit(const Solver &s, const char *who, const GraphFactors &f, const std::vector<double> &more) {
    std::vector<double> units(f.unit);
    units.insert(units.end(), more.begin(), more.end());
    for (double u : units)
      if (u != units[0]) {
        std::ostringstream m;
        m << who << ": the factors and candidates were given with sigma_pixel = " << units[0] / s.scaler_ << " and "
          << u / s.scaler_ << "; a covariance in the caller's units needs one value";
        throw std::runtime_error(m.str());
      }
    return units.empty() ? static_cast<double>(s.scaler_) : units[0];
  }

  static int32_t PoseIndex(const Solver &s, _BA_Pose *pose) {
    const auto it = s.pose_index_.find(pose);
    if (it == s.pose_index_.end()) throw std::runtime_error("There is no pointer in the BA pose pool.");
    return static_cast<int32_t>(it->second);
  }

  // solve, the solved poses, the factor report into f->report_* in the caller's units
  static void Run(const Solver &s, const char *who, GraphFactors *f, const Options &options, GraphRun *run) {
    const ba_options o = PackOptions(options, s.gauss_newton_);
    run->rows.resize(static_cast<size_t>(std::max(1, o.max_num_iterations)));
    run->solved.resize(Abi::kPose * s.poses_.size());
    std::vector<double> rep_s(f->j.size()), rep_w(f->j.size());
    {
      const GraphSession<Abi> g = Open(s, who, *f, &run->start);
      g.Check(Abi::solve(g.get(), &o, run->rows.data(), static_cast<int>(run->rows.size()), &run->n_iter,
                         &run->converged),
              "solve");
      g.Check(Abi::get_poses(g.get(), run->solved.data()), "get_poses");
      const char *entry = nullptr;
      const int rc = Abi::FactorReport(g.get(), f->kind, rep_s.data(), &rep_w, &entry);
      g.Check(rc, entry);
    }
    for (size_t i = 0; i < rep_s.size(); ++i) rep_s[i] /= f->unit[i] * f->unit[i];  // the caller's units
    f->report_s.swap(rep_s);
    f->report_w.swap(rep_w);
  }

  static bool Covariance(const Solver &s, const char *who, const GraphFactors &f, const std::vector<_BA_Pose *> &poses,
                         const std::vector<std::pair<_BA_Pose *, _BA_Pose *>> &pairs, std::vector<Block> *cov_poses,
                         std::vector<Block> *cov_cross, std::vector<Block> *cov_rel) {
    constexpr int W = Abi::kWidth, WW = W * W;
    const double unit = Unit(s, who, f, {});
    std::vector<int32_t> ps, pj, pk;
    for (_BA_Pose *p : poses) ps.push_back(PoseIndex(s, p));
    for (const auto &jk : pairs) {
      pj.push_back(PoseIndex(s, jk.first));
      pk.push_back(PoseIndex(s, jk.second));
    }
    if ((!ps.empty() && cov_poses == nullptr) || (!pj.empty() && cov_rel == nullptr))
      throw std::runtime_error(std::string(who) + ": null output for a non-empty selection");
    std::vector<double> cp(WW * ps.size()), cc(WW * pj.size()), cr(WW * pj.size());
    int64_t dropped = 0;
    {
      const GraphSession<Abi> g = Open(s, who, f);
      if (Abi::covariance(g.get(), static_cast<int>(ps.size()), ps.empty() ? nullptr : ps.data(),
                          ps.empty() ? nullptr : cp.data(), static_cast<int64_t>(pj.size()),
                          pj.empty() ? nullptr : pj.data(), pj.empty() ? nullptr : pk.data(),
                          pj.empty() || cov_cross == nullptr ? nullptr : cc.data(), pj.empty() ? nullptr : cr.data(),
                          &dropped) != 0)
        throw std::runtime_error(Abi::last_error());
    }
    // scaled units -> the caller's: Sigma_user = unit^2 D Sigma_scaled D, D = diag(100 I3, I)
    const auto to_user = [&](const std::vector<double> &in, std::vector<Block> *out) {
      if (out == nullptr) return;
      out->resize(in.size() / WW);
      for (size_t b = 0; b < out->size(); ++b)
        for (int r = 0; r < W; ++r)
          for (int c = 0; c < W; ++c) {
            const double dr = r < 3 ? static_cast<double>(s.inverse_scaler_) : 1.0;
            const double dc = c < 3 ? static_cast<double>(s.inverse_scaler_) : 1.0;
            (*out)[b](r, c) = (unit * unit) * (dr * in[WW * b + W * r + c] * dc);
          }
    };
    to_user(cp, cov_poses);
    to_user(cc, cov_cross);
    to_user(cr, cov_rel);
    return dropped == 0;
  }

  // pack(&c): the n candidates into c.j, c.k, c.Z, c.Omega, the kind's own way
  template <class Pack>
  static bool Gate(const Solver &s, const char *who, const GraphFactors &f, size_t n, double sigma_pixel,
                   std::vector<double> *d2, Pack pack) {
    if (d2 == nullptr) throw std::runtime_error(std::string(who) + ": null output");
    const double unit = Unit(s, who, f, std::vector<double>(n, sigma_pixel * static_cast<double>(s.scaler_)));
    RelativeArrays c;
    pack(&c);
    d2->assign(n, 0.0);
    int64_t dropped = 0;
    {
      const GraphSession<Abi> g = Open(s, who, f);
      const bool any = n != 0;
      if (Abi::gate(g.get(), static_cast<int64_t>(n), any ? c.j.data() : nullptr, any ? c.k.data() : nullptr,
                    any ? c.Z.data() : nullptr, any ? c.Omega.data() : nullptr, any ? d2->data() : nullptr, nullptr,
                    nullptr, &dropped) != 0)
        throw std::runtime_error(Abi::last_error());
    }
    for (double &v : *d2) v /= unit * unit;  // d2_user = d2_scaled / unit^2
    return dropped == 0;
  }

  static void Weights(const char *who, const char *solve, const GraphFactors &f, std::vector<double> *s,
                      std::vector<double> *w) {
    if (f.report_w.empty()) throw std::runtime_error(std::string(who) + ": " + solve + " has not run");
    if (s != nullptr) *s = f.report_s;
    if (w != nullptr) *w = f.report_w;
  }
};

// ---- SE(3): the factors of AddRelativePose ----
bool FullBundleAdjustmentSolver::SolvePoseGraph(Options options, Summary *summary) {
  timer::StopWatch stopwatch("BundleAdjustmentSolver::SolvePoseGraph");
  stopwatch.Start();
  BeginSummary(summary, options);
  GraphRun run;
  Graph<Se3Abi>::Run(*this, "SolvePoseGraph", &relatives_, options, &run);
  const std::vector<uint8_t> no_point(points_.size(), 0);
  WriteBack(run.solved.data(), nullptr, no_point.data());
  FinishSummary(summary, run.rows, run.n_iter, run.converged, stopwatch);
  return true;
}

void FullBundleAdjustmentSolver::GetRelativeWeights(std::vector<double> *s, std::vector<double> *w) const {
  Graph<Se3Abi>::Weights("GetRelativeWeights", "SolvePoseGraph", relatives_, s, w);
}

bool FullBundleAdjustmentSolver::ComputePoseGraphCovariance(const std::vector<_BA_Pose *> &poses,
                                                            const std::vector<std::pair<_BA_Pose *, _BA_Pose *>> &pairs,
                                                            std::vector<Eigen::Matrix<double, 6, 6>> *cov_poses,
                                                            std::vector<Eigen::Matrix<double, 6, 6>> *cov_cross,
                                                            std::vector<Eigen::Matrix<double, 6, 6>> *cov_rel) {
  return Graph<Se3Abi>::Covariance(*this, "ComputePoseGraphCovariance", relatives_, poses, pairs, cov_poses, cov_cross,
                                   cov_rel);
}

bool FullBundleAdjustmentSolver::GateLoopClosures(const std::vector<RelativePose> &candidates, double sigma_pixel,
                                                  std::vector<double> *d2) {
  const char *who = "GateLoopClosures";
  return Graph<Se3Abi>::Gate(*this, who, relatives_, candidates.size(), sigma_pixel, d2, [&](RelativeArrays *c) {
    const std::vector<std::vector<RelativePose>> lists(1, candidates);
    PackRelatives({this}, who, &lists, sigma_pixel, c);  // throws on a candidate that carries a kernel
  });
}

// ---- Sim(3): the factors of AddRelativeSim3 ----
void FullBundleAdjustmentSolver::PackSim3(const RelativeSim3 &f, double sigma_pixel, std::vector<double> *Z,
                                          std::vector<double> *Omega) const {
  const double *M = f.measurement;
  const double det = M[0] * (M[5] * M[10] - M[6] * M[9]) - M[1] * (M[4] * M[10] - M[6] * M[8]) +
                     M[2] * (M[4] * M[9] - M[5] * M[8]);
  const double s = std::cbrt(det);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) Z->push_back(M[4 * r + c] / s);
  for (int r = 0; r < 3; ++r) Z->push_back(M[4 * r + 3] * static_cast<double>(scaler_));
  Z->push_back(s);
  // the caller's units -> scaled units, unit pixel noise: as PackRelatives converts the 6x6
  const double w = 1.0 / (sigma_pixel * sigma_pixel * static_cast<double>(scaler_) * static_cast<double>(scaler_));
  const auto d = [this](int r) { return r < 3 ? static_cast<double>(inverse_scaler_) : 1.0; };
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c) Omega->push_back((d(r) * f.information[7 * r + c] * d(c)) / w);
}

void FullBundleAdjustmentSolver::AddRelativeSim3(const RelativeSim3 &f, double sigma_pixel) {
  const auto ij = pose_index_.find(f.pose_j), ik = pose_index_.find(f.pose_k);
  if (ij == pose_index_.end() || ik == pose_index_.end())
    throw std::runtime_error("AddRelativeSim3: there is no pointer in the BA pose pool.");
  const double unit = sigma_pixel * static_cast<double>(scaler_);
  int32_t kind = 0;
  double scale = 0.0;
  if (f.robust_kind != 0) {
    kind = f.robust_kind;
    if (ba_sim3_robust_check(1, &kind, &f.robust_scale) != 0)
      throw std::runtime_error(std::string("AddRelativeSim3: ") + ba_last_error());
    scale = f.robust_scale * unit;  // s in scaled units is s in the caller's units times unit^2
  }
  sim3_.j.push_back(ij->second);
  sim3_.k.push_back(ik->second);
  PackSim3(f, sigma_pixel, &sim3_.Z, &sim3_.Omega);
  sim3_.kind.push_back(kind);
  sim3_.scale.push_back(scale);
  sim3_.unit.push_back(unit);
}

bool FullBundleAdjustmentSolver::SolveSim3Graph(Options options, Summary *summary,
                                                const std::vector<int> *point_anchors, std::vector<double> *scales) {
  timer::StopWatch stopwatch("BundleAdjustmentSolver::SolveSim3Graph");
  stopwatch.Start();
  BeginSummary(summary, options);
  Graph<Sim3Abi>::Require(*this, "SolveSim3Graph", sim3_);  // before the anchors are looked at
  const size_t n_pose = poses_.size(), n_pt = points_.size();
  if (point_anchors != nullptr) {
    if (point_anchors->size() != n_pt) throw std::runtime_error("SolveSim3Graph: one anchor (or -1) per registered point");
    for (int a : *point_anchors)
      if (a >= static_cast<int>(n_pose)) throw std::runtime_error("SolveSim3Graph: an anchor is no registered pose");
  }
  GraphRun run;
  Graph<Sim3Abi>::Run(*this, "SolveSim3Graph", &sim3_, options, &run);
  const std::vector<double> &S = run.start, &S_new = run.solved;
  // rigid poses T_jw = [R, t / s]; the anchored points follow their keyframes
  std::vector<double> T(12 * n_pose), X(3 * n_pt, 0.0);
  std::vector<uint8_t> moved(n_pt, 0);
  for (size_t p = 0; p < n_pose; ++p) {
    const double s = S_new[13 * p + 12];
    for (int e = 0; e < 9; ++e) T[12 * p + e] = S_new[13 * p + e];
    for (int e = 9; e < 12; ++e) T[12 * p + e] = S_new[13 * p + e] / s;
  }
  for (size_t q = 0; point_anchors != nullptr && q < n_pt; ++q) {
    const int a = (*point_anchors)[q];
    if (a < 0 || fixed_points_.count(static_cast<int>(q))) continue;
    const double *So = &S[13 * static_cast<size_t>(a)], *Sn = &S_new[13 * static_cast<size_t>(a)];
    double Y[3];
    for (int r = 0; r < 3; ++r)  // T_old,a X, then over the new scale
      Y[r] = ((So[3 * r] * X_[q](0) + So[3 * r + 1] * X_[q](1) + So[3 * r + 2] * X_[q](2) + So[9 + r]) - Sn[9 + r]) /
             Sn[12];
    for (int r = 0; r < 3; ++r) X[3 * q + r] = Sn[r] * Y[0] + Sn[3 + r] * Y[1] + Sn[6 + r] * Y[2];  // R_new^T
    moved[q] = 1;
  }
  WriteBack(T.data(), X.data(), moved.data());
  if (scales != nullptr) {
    scales->resize(n_pose);
    for (size_t p = 0; p < n_pose; ++p) (*scales)[p] = S_new[13 * p + 12];
  }
  FinishSummary(summary, run.rows, run.n_iter, run.converged, stopwatch);
  return true;
}

void FullBundleAdjustmentSolver::GetRelativeSim3Weights(std::vector<double> *s, std::vector<double> *w) const {
  Graph<Sim3Abi>::Weights("GetRelativeSim3Weights", "SolveSim3Graph", sim3_, s, w);
}

bool FullBundleAdjustmentSolver::ComputeSim3GraphCovariance(const std::vector<_BA_Pose *> &poses,
                                                            const std::vector<std::pair<_BA_Pose *, _BA_Pose *>> &pairs,
                                                            std::vector<Eigen::Matrix<double, 7, 7>> *cov_poses,
                                                            std::vector<Eigen::Matrix<double, 7, 7>> *cov_cross,
                                                            std::vector<Eigen::Matrix<double, 7, 7>> *cov_rel) {
  return Graph<Sim3Abi>::Covariance(*this, "ComputeSim3GraphCovariance", sim3_, poses, pairs, cov_poses, cov_cross,
                                    cov_rel);
}

bool FullBundleAdjustmentSolver::GateSim3LoopClosures(const std::vector<RelativeSim3> &candidates, double sigma_pixel,
                                                      std::vector<double> *d2) {
  const char *who = "GateSim3LoopClosures";
  return Graph<Sim3Abi>::Gate(*this, who, sim3_, candidates.size(), sigma_pixel, d2, [&](RelativeArrays *c) {
    for (const RelativeSim3 &cand : candidates) {  // a candidate's kernel is not read
      c->j.push_back(Graph<Sim3Abi>::PoseIndex(*this, cand.pose_j));
      c->k.push_back(Graph<Sim3Abi>::PoseIndex(*this, cand.pose_k));
      PackSim3(cand, sigma_pixel, &c->Z, &c->Omega);
    }
  });
}

bool FullBundleAdjustmentSolver::ComputeCovariance(const std::vector<_BA_Pose *> &poses,
                                                   const std::vector<_BA_Point *> &points, double sigma_pixel,
                                                   std::vector<Eigen::Matrix<double, 6, 6>> *cov_poses,
                                                   std::vector<Eigen::Matrix<double, 3, 3>> *cov_points) {
  std::vector<int32_t> ps, qs;
  for (_BA_Pose *p : poses) {
    const auto it = pose_index_.find(p);
    if (it == pose_index_.end()) throw std::runtime_error("There is no pointer in the BA pose pool.");
    if (fixed_poses_.count(it->second)) throw std::runtime_error("ComputeCovariance: a fixed pose has no covariance.");
    ps.push_back(it->second);
  }
  for (_BA_Point *q : points) {
    const auto it = point_index_.find(q);
    if (it == point_index_.end()) throw std::runtime_error("There is no pointer in the BA point pool.");
    if (fixed_points_.count(it->second)) throw std::runtime_error("ComputeCovariance: a fixed point has no covariance.");
    qs.push_back(it->second);
  }
  if ((!ps.empty() && cov_poses == nullptr) || (!qs.empty() && cov_points == nullptr))
    throw std::runtime_error("ComputeCovariance: null output for a non-empty selection");
  FinalizeParameters();
  std::vector<double> cp(36 * ps.size()), cq(9 * qs.size());
  int64_t dropped = 0;
  const Options defaults;
  Check(ba_covariance(handle_, static_cast<double>(defaults.outlier_handle.threshold_huber_loss),
                      static_cast<int>(ps.size()), ps.empty() ? nullptr : ps.data(), ps.empty() ? nullptr : cp.data(),
                      static_cast<int>(qs.size()), qs.empty() ? nullptr : qs.data(), qs.empty() ? nullptr : cq.data(),
                      &dropped),
        "ba_covariance");
  // scaled units, unit pixel noise -> the caller's units (see the header)
  const double s2 = sigma_pixel * sigma_pixel;
  const double k_pose = s2 * static_cast<double>(scaler_) * static_cast<double>(scaler_);
  if (cov_poses != nullptr) {
    cov_poses->resize(ps.size());
    for (size_t s = 0; s < ps.size(); ++s)
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
          const double dr = r < 3 ? static_cast<double>(inverse_scaler_) : 1.0;
          const double dc = c < 3 ? static_cast<double>(inverse_scaler_) : 1.0;
          (*cov_poses)[s](r, c) = k_pose * (dr * cp[36 * s + 6 * r + c] * dc);
        }
  }
  if (cov_points != nullptr) {
    cov_points->resize(qs.size());
    for (size_t s = 0; s < qs.size(); ++s)
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) (*cov_points)[s](r, c) = s2 * cq[9 * s + 3 * r + c];
  }
  return dropped == 0;
}

void FullBundleAdjustmentSolver::PackBatch(const std::vector<FullBundleAdjustmentSolver *> &solvers, const char *who,
                                           bool check_connectivity, BatchArrays *out) {
  BatchArrays &a = *out;
  a.cam_off.assign(1, 0);
  a.pose_off.assign(1, 0);
  a.pt_off.assign(1, 0);
  a.obs_off.assign(1, 0);
  const std::string name(who);
  for (FullBundleAdjustmentSolver *s : solvers) {
    if (s == nullptr) throw std::runtime_error(name + ": null solver");
    if (s->shard_world_ > 1 || s->allreduce_fn_) throw std::runtime_error(name + ": a sharded solver cannot join a batch");
    if (s->cameras_.empty() || s->poses_.empty() || s->points_.empty())
      throw std::runtime_error(name + ": cameras, poses and points must be added first");
    if (check_connectivity) s->CheckPoseAndPointConnectivity();
    for (size_t c = 0; c < s->cameras_.size(); ++c) {
      a.intr.insert(a.intr.end(), {s->cameras_[c].fx, s->cameras_[c].fy, s->cameras_[c].cx, s->cameras_[c].cy});
      a.T_cj.resize(a.T_cj.size() + 12);
      Pack12(s->cameras_[c].pose_this_to_cam0, &a.T_cj[a.T_cj.size() - 12]);
    }
    for (size_t p = 0; p < s->poses_.size(); ++p) {
      a.T.resize(a.T.size() + 12);
      Pack12(s->T_jw_[p], &a.T[a.T.size() - 12]);
      a.pose_fixed.push_back(s->fixed_poses_.count(static_cast<int>(p)) > 0);
    }
    for (size_t q = 0; q < s->points_.size(); ++q) {
      for (int r = 0; r < 3; ++r) a.X.push_back(s->X_[q](r));
      a.point_fixed.push_back(s->fixed_points_.count(static_cast<int>(q)) > 0);
    }
    for (const Observation &o : s->observations_) {  // insertion order matters (:826)
      a.oc.push_back(o.camera_index);
      a.op.push_back(o.pose_index);
      a.oq.push_back(o.point_index);
      a.uv.push_back(o.u);
      a.uv.push_back(o.v);
    }
    a.cam_off.push_back(static_cast<int32_t>(a.intr.size() / 4));
    a.pose_off.push_back(static_cast<int32_t>(a.pose_fixed.size()));
    a.pt_off.push_back(static_cast<int32_t>(a.point_fixed.size()));
    a.obs_off.push_back(static_cast<int64_t>(a.oc.size()));
  }
}

int FullBundleAdjustmentSolver::CreateBatch(const BatchArrays &a, int device, ba_handle **h, ba_batch **batch) {
  Check(ba_create(h, device), "ba_create");
  return ba_batch_create(batch, *h, static_cast<int>(a.obs_off.size()) - 1, a.cam_off.data(), a.pose_off.data(),
                         a.pt_off.data(), a.obs_off.data(), a.intr.data(), a.T_cj.data(), a.T.data(),
                         a.pose_fixed.data(), a.X.data(), a.point_fixed.data(), a.oc.data(), a.op.data(), a.oq.data(),
                         a.uv.data());
}

int FullBundleAdjustmentSolver::SetPriors(ba_batch *batch, const PriorArrays &p) {
  if (!p.set) return 0;
  return ba_batch_set_prior(batch, p.off.data(), p.pose.data(), p.T_lin.data(), p.H.data(), p.b.data(), p.c.data());
}

void FullBundleAdjustmentSolver::PackPriors(const std::vector<FullBundleAdjustmentSolver *> &solvers, const char *who,
                                            const std::vector<PosePrior> *in_priors, double sigma_pixel,
                                            PriorArrays *out) {
  if (in_priors == nullptr) return;
  const std::string name(who);
  if (in_priors->size() != solvers.size()) throw std::runtime_error(name + ": one prior per solver");
  out->set = true;
  std::vector<int32_t> &off = out->off, &pose = out->pose;
  std::vector<double> &Tl = out->T_lin, &H = out->H, &bv = out->b, &cs = out->c;
  off.assign(1, 0);
  for (size_t k = 0; k < solvers.size(); ++k) {
    const FullBundleAdjustmentSolver *s = solvers[k];
    const PosePrior &p = (*in_priors)[k];
    const size_t K = p.poses.size(), n = 6 * K;
    if (p.H.size() != n * n || p.b.size() != n || p.lin_poses.size() != K)
      throw std::runtime_error(name + ": a prior needs H (6K x 6K), b (6K) and K lin_poses");
    // registration order (ascending index), the blocks of H and b permuted with the poses
    std::vector<std::pair<int, int>> order;  // (registration index, position in the prior)
    for (size_t t = 0; t < K; ++t) {
      const auto it = s->pose_index_.find(p.poses[t]);
      if (it == s->pose_index_.end()) throw std::runtime_error(name + ": there is no pointer in the BA pose pool.");
      order.emplace_back(it->second, static_cast<int>(t));
    }
    std::sort(order.begin(), order.end());
    // the caller's units -> scaled units, unit pixel noise: the inverse of MarginalizeBatch's
    const double w = 1.0 / (sigma_pixel * sigma_pixel * static_cast<double>(s->scaler_) * static_cast<double>(s->scaler_));
    const auto d = [s](size_t r) { return r % 6 < 3 ? static_cast<double>(s->inverse_scaler_) : 1.0; };
    for (size_t t = 0; t < K; ++t) {
      pose.push_back(order[t].first);
      _BA_Pose T_jw = p.lin_poses[static_cast<size_t>(order[t].second)].inverse();
      T_jw.translation() = T_jw.translation() * s->scaler_;
      Tl.resize(Tl.size() + 12);
      Pack12(T_jw, &Tl[Tl.size() - 12]);
    }
    for (size_t r = 0; r < n; ++r) {
      const size_t sr = 6 * static_cast<size_t>(order[r / 6].second) + r % 6;
      for (size_t c = 0; c < n; ++c) {
        const size_t sc = 6 * static_cast<size_t>(order[c / 6].second) + c % 6;
        H.push_back((d(r) * p.H[sr * n + sc] * d(c)) / w);
      }
      bv.push_back((d(r) * p.b[sr]) / w);
    }
    cs.push_back(p.c / w);
    off.push_back(static_cast<int32_t>(pose.size()));
  }
}

int FullBundleAdjustmentSolver::SetRelatives(ba_batch *batch, const RelativeArrays &r) {
  if (!r.set) return 0;
  return ba_batch_set_relative(batch, r.off.data(), r.j.data(), r.k.data(), r.Z.data(), r.Omega.data());
}

void FullBundleAdjustmentSolver::PackRelatives(const std::vector<FullBundleAdjustmentSolver *> &solvers,
                                               const char *who,
                                               const std::vector<std::vector<RelativePose>> *in_relatives,
                                               double sigma_pixel, RelativeArrays *out) {
  if (in_relatives == nullptr) return;
  const std::string name(who);
  if (in_relatives->size() != solvers.size())
    throw std::runtime_error(name + ": one list of relative-pose factors per solver");
  out->set = true;
  out->off.assign(1, 0);
  for (size_t b = 0; b < solvers.size(); ++b) {
    const FullBundleAdjustmentSolver *s = solvers[b];
    // the caller's units -> scaled units, unit pixel noise: as PackPriors converts a 6x6 H
    const double w = 1.0 / (sigma_pixel * sigma_pixel * static_cast<double>(s->scaler_) * static_cast<double>(s->scaler_));
    const auto d = [s](int r) { return r < 3 ? static_cast<double>(s->inverse_scaler_) : 1.0; };
    for (const RelativePose &f : (*in_relatives)[b]) {
      // s in scaled units = s in the caller's units times unit^2: the scale goes in times unit
      const double unit = sigma_pixel * static_cast<double>(s->scaler_);
      int32_t kind = 0;
      double scale = 0.0;
      if (f.robust_kind != 0) {
        if (name != "AddRelativePose")
          throw std::runtime_error(name + ": factor " + std::to_string(out->j.size() - out->off.back()) +
                                   " carries a robust kernel; robust factors are pose-graph only (AddRelativePose + "
                                   "SolvePoseGraph)");
        kind = f.robust_kind;
        if (ba_pgraph_robust_check(1, &kind, &f.robust_scale) != 0)
          throw std::runtime_error(name + ": " + ba_last_error());
        scale = f.robust_scale * unit;
      }
      out->kind.push_back(kind);
      out->scale.push_back(scale);
      out->unit.push_back(unit);
      const auto ij = s->pose_index_.find(f.pose_j), ik = s->pose_index_.find(f.pose_k);
      if (ij == s->pose_index_.end() || ik == s->pose_index_.end())
        throw std::runtime_error(name + ": there is no pointer in the BA pose pool.");
      out->j.push_back(ij->second);
      out->k.push_back(ik->second);
      _BA_Pose Z = f.measurement;
      Z.translation() = Z.translation() * s->scaler_;
      out->Z.resize(out->Z.size() + 12);
      Pack12(Z, &out->Z[out->Z.size() - 12]);
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) out->Omega.push_back((d(r) * f.information[6 * r + c] * d(c)) / w);
    }
    out->off.push_back(static_cast<int32_t>(out->j.size()));
  }
  // a batch without any factor still needs addressable arrays
  if (out->j.empty()) {
    out->j.assign(1, 0);
    out->k.assign(1, 0);
    out->Z.assign(12, 0.0);
    out->Omega.assign(36, 0.0);
  }
}

bool FullBundleAdjustmentSolver::PackMasks(const BatchArrays &a, const char *who,
                                           const std::vector<std::vector<uint8_t>> *obs_masks,
                                           std::vector<uint8_t> *flat) {
  if (obs_masks == nullptr) return false;
  const size_t B = a.obs_off.size() - 1;
  if (obs_masks->size() != B) throw std::runtime_error(std::string(who) + ": one observation mask per solver");
  flat->assign(static_cast<size_t>(a.obs_off[B]), 1);
  for (size_t b = 0; b < B; ++b) {
    const std::vector<uint8_t> &m = (*obs_masks)[b];
    const size_t n = static_cast<size_t>(a.obs_off[b + 1] - a.obs_off[b]);
    if (m.empty()) continue;
    if (m.size() != n)
      throw std::runtime_error(std::string(who) + ": solver " + std::to_string(b) + " registered " +
                               std::to_string(n) + " observations, its mask holds " + std::to_string(m.size()) +
                               " flags");
    for (size_t k = 0; k < n; ++k) (*flat)[static_cast<size_t>(a.obs_off[b]) + k] = m[k] ? 1 : 0;
  }
  return true;
}

bool FullBundleAdjustmentSolver::SolveBatch(const std::vector<FullBundleAdjustmentSolver *> &solvers, Options options,
                                            std::vector<Summary> *summaries, const std::vector<PosePrior> *in_priors,
                                            double sigma_pixel,
                                            const std::vector<std::vector<RelativePose>> *in_relatives,
                                            const std::vector<std::vector<uint8_t>> *obs_masks,
                                            const CullOptions *cull, std::vector<CullReport> *cull_reports) {
  timer::StopWatch stopwatch("BundleAdjustmentSolver::SolveBatch");
  stopwatch.Start();
  const int B = static_cast<int>(solvers.size());
  if (summaries != nullptr) summaries->assign(static_cast<size_t>(B), Summary());
  if (B == 0) return true;
  BatchArrays a;
  PackBatch(solvers, "SolveBatch", true, &a);
  PriorArrays pa;
  PackPriors(solvers, "SolveBatch", in_priors, sigma_pixel, &pa);
  RelativeArrays ra;
  PackRelatives(solvers, "SolveBatch", in_relatives, sigma_pixel, &ra);
  std::vector<int32_t> &pose_off = a.pose_off, &pt_off = a.pt_off;
  std::vector<double> &T = a.T, &X = a.X;
  std::vector<uint8_t> mask;
  const bool masked = PackMasks(a, "SolveBatch", obs_masks, &mask);
  const ba_options o = PackOptions(options, solvers[0]->gauss_newton_);
  // with cull: the rows of stage 1, then those of stage 2 from row `first_iters` on
  ba_options o_first = o;
  ba_cull_options co{0.0, 0};
  int first_iters = 0;
  if (cull != nullptr) {
    o_first = PackOptions(cull->first, solvers[0]->gauss_newton_);
    const double sc = static_cast<double>(solvers[0]->scaler_);
    co.e2_max = cull->chi2 * sigma_pixel * sigma_pixel * sc * sc;
    co.cull_behind = cull->cull_behind ? 1 : 0;
    if (ba_batch_cull_check(&co) != 0) throw std::runtime_error(std::string("SolveBatch failed: ") + ba_last_error());
    if (o_first.max_num_iterations <= 0 || o.max_num_iterations <= 0)
      throw std::runtime_error("SolveBatch: with cull both stages need max_num_iterations >= 1");
    first_iters = o_first.max_num_iterations;
  }
  if (cull_reports != nullptr) cull_reports->assign(static_cast<size_t>(cull ? B : 0), CullReport());
  const int cap = first_iters + std::max(1, o.max_num_iterations);
  std::vector<ba_iter_info> rows(static_cast<size_t>(B) * cap);
  std::vector<ba_batch_result> res(static_cast<size_t>(B)), res_first(static_cast<size_t>(B));
  std::vector<ba_batch_cull_result> cres(static_cast<size_t>(B));
  ba_handle *h = nullptr;
  ba_batch *batch = nullptr;
  int rc = CreateBatch(a, solvers[0]->device_id_, &h, &batch);
  if (rc == 0) rc = SetPriors(batch, pa);
  if (rc == 0) rc = SetRelatives(batch, ra);
  if (rc == 0 && masked) rc = ba_batch_set_obs_mask(batch, mask.data());
  if (rc == 0 && cull == nullptr) rc = ba_batch_solve(batch, &o, rows.data(), cap, res.data());
  if (rc == 0 && cull != nullptr) {
    rc = ba_batch_solve_culled(batch, &o_first, &o, &co, rows.data(), cap, res_first.data(), res.data(), cres.data());
    if (rc == 0 && cull_reports != nullptr) {
      mask.assign(static_cast<size_t>(a.obs_off[B]), 1);
      rc = ba_batch_get_obs_mask(batch, mask.data());
      for (int b = 0; rc == 0 && b < B; ++b) {
        CullReport &r = (*cull_reports)[b];
        r.inliers.assign(mask.begin() + a.obs_off[b], mask.begin() + a.obs_off[b + 1]);
        r.n_culled = cres[b].n_culled;
        r.starved = cres[b].starved;
        r.n_iter_first = res_first[b].n_iter;
      }
    }
  }
  if (rc == 0) rc = ba_batch_get_poses(batch, T.data());
  if (rc == 0) rc = ba_batch_get_points(batch, X.data());
  const std::string err = rc ? ba_last_error() : "";
  ba_batch_destroy(batch);
  ba_destroy(h);
  if (rc) throw std::runtime_error("SolveBatch failed: " + err);
  bool all_solved = true;
  for (int b = 0; b < B; ++b) {
    FullBundleAdjustmentSolver *s = solvers[b];
    Summary *summary = summaries ? &(*summaries)[b] : nullptr;
    BeginSummary(summary, options);
    if (summary != nullptr) summary->convergence_status_ = res[b].status == 0 && res[b].converged != 0;
    if (res[b].status != 0) {
      all_solved = false;
      continue;
    }
    const double *Tb = &T[12 * static_cast<size_t>(pose_off[b])], *Xb = &X[3 * static_cast<size_t>(pt_off[b])];
    const std::vector<uint8_t> valid(s->points_.size(), 1);
    s->WriteBack(Tb, Xb, valid.data());
    // a finalized solver continues from the solution, as after Solve
    if (s->is_parameter_finalized_) Check(ba_update_values(s->handle_, Tb, Xb), "ba_update_values");
    if (summary != nullptr) {
      for (int k = 0; cull != nullptr && k < res_first[b].n_rows && k < first_iters; ++k)
        summary->optimization_info_list_.push_back(ToInfo(rows[static_cast<size_t>(b) * cap + k]));
      for (int k = 0; k < res[b].n_rows && first_iters + k < cap; ++k)
        summary->optimization_info_list_.push_back(ToInfo(rows[static_cast<size_t>(b) * cap + first_iters + k]));
      summary->total_time_in_millisecond_ = stopwatch.GetLapTimeFromStart();
    }
  }
  return all_solved;
}

bool FullBundleAdjustmentSolver::SolvePointsOnly(Options options, std::vector<PointOnlyResult> *results,
                                                 const std::vector<_BA_Point *> &triangulate) {
  if (results != nullptr) results->clear();
  if (shard_world_ > 1 || allreduce_fn_) throw std::runtime_error("SolvePointsOnly: not available on a sharded solver");
  if (cameras_.empty() || poses_.empty() || points_.empty())
    throw std::runtime_error("SolvePointsOnly: cameras, poses and points must be added first");
  std::vector<uint8_t> tri_all(points_.size(), 0);
  for (_BA_Point *q : triangulate) {
    const auto it = point_index_.find(q);
    if (it == point_index_.end()) throw std::runtime_error("There is no pointer in the BA point pool.");
    if (fixed_points_.count(it->second)) throw std::runtime_error("SolvePointsOnly: a fixed point is not triangulated.");
    tri_all[static_cast<size_t>(it->second)] = 1;
  }
  // the non-fixed points in registration order, their observations landmark-major (stable)
  std::vector<int> sel, new_of(points_.size(), -1);
  for (size_t q = 0; q < points_.size(); ++q)
    if (!fixed_points_.count(static_cast<int>(q))) {
      new_of[q] = static_cast<int>(sel.size());
      sel.push_back(static_cast<int>(q));
    }
  const int n_pt = static_cast<int>(sel.size());
  if (n_pt == 0) return true;
  std::vector<int64_t> off(static_cast<size_t>(n_pt) + 1, 0);
  for (const Observation &o : observations_)
    if (new_of[o.point_index] >= 0) ++off[static_cast<size_t>(new_of[o.point_index]) + 1];
  for (int i = 0; i < n_pt; ++i) off[i + 1] += off[i];
  const size_t n_obs = static_cast<size_t>(off[n_pt]);
  std::vector<int32_t> oc(std::max<size_t>(n_obs, 1)), op(std::max<size_t>(n_obs, 1));
  std::vector<double> uv(2 * std::max<size_t>(n_obs, 1));
  std::vector<int64_t> at(off.begin(), off.end() - 1);
  for (const Observation &o : observations_) {
    const int i = new_of[o.point_index];
    if (i < 0) continue;
    const size_t k = static_cast<size_t>(at[i]++);
    oc[k] = o.camera_index;
    op[k] = o.pose_index;
    uv[2 * k] = o.u;
    uv[2 * k + 1] = o.v;
  }
  std::vector<double> intr(4 * cameras_.size()), T_cj(12 * cameras_.size()), T(12 * poses_.size()),
      X(3 * static_cast<size_t>(n_pt));
  for (size_t c = 0; c < cameras_.size(); ++c) {
    intr[4 * c + 0] = cameras_[c].fx;
    intr[4 * c + 1] = cameras_[c].fy;
    intr[4 * c + 2] = cameras_[c].cx;
    intr[4 * c + 3] = cameras_[c].cy;
    Pack12(cameras_[c].pose_this_to_cam0, &T_cj[12 * c]);
  }
  for (size_t p = 0; p < poses_.size(); ++p) Pack12(T_jw_[p], &T[12 * p]);
  std::vector<uint8_t> tri(static_cast<size_t>(n_pt));
  for (int i = 0; i < n_pt; ++i) {
    for (int r = 0; r < 3; ++r) X[3 * i + r] = X_[sel[i]](r);
    tri[i] = tri_all[sel[i]];
  }
  const ba_options o = PackOptions(options, gauss_newton_);
  std::vector<ba_point_result> res(static_cast<size_t>(n_pt));
  ba_handle *h = handle_;
  if (h == nullptr && ba_create(&h, device_id_) != 0)
    throw std::runtime_error(std::string("SolvePointsOnly: ba_create failed: ") + ba_last_error());
  const int rc = ba_point_only(h, static_cast<int>(cameras_.size()), intr.data(), T_cj.data(),
                               static_cast<int>(poses_.size()), T.data(), n_pt, off.data(), oc.data(), op.data(),
                               uv.data(), tri.data(), X.data(), &o, nullptr, 0, res.data());
  const std::string err = rc ? ba_last_error() : "";
  if (h != handle_) ba_destroy(h);
  if (rc) throw std::runtime_error("SolvePointsOnly failed: " + err);
  bool all_solved = true;
  for (int i = 0; i < n_pt; ++i) {
    const size_t q = static_cast<size_t>(sel[i]);
    if (res[i].status == 0) {
      X_[q] = _BA_Point(X[3 * i], X[3 * i + 1], X[3 * i + 2]);
      *points_[q] = X_[q] * inverse_scaler_;
    } else {
      all_solved = false;
    }
    if (results != nullptr) {
      PointOnlyResult r;
      r.point = points_[q];
      r.n_iter = res[i].n_iter;
      r.converged = res[i].converged;
      r.status = res[i].status;
      r.n_behind = res[i].n_behind;
      r.dropped_pivots = res[i].dropped_pivots;
      r.cost0 = res[i].cost0;
      r.cost = res[i].cost;
      results->push_back(r);
    }
  }
  if (is_parameter_finalized_) {  // a finalized solver continues from the new points
    std::vector<double> Xall(3 * points_.size());
    for (size_t q = 0; q < points_.size(); ++q)
      for (int r = 0; r < 3; ++r) Xall[3 * q + r] = X_[q](r);
    Check(ba_update_values(handle_, nullptr, Xall.data()), "ba_update_values");
  }
  return all_solved;
}

bool FullBundleAdjustmentSolver::ComputeCovarianceBatch(
    const std::vector<FullBundleAdjustmentSolver *> &solvers, double sigma_pixel,
    std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> *cov_poses,
    std::vector<std::vector<Eigen::Matrix<double, 3, 3>>> *cov_points, const std::vector<PosePrior> *in_priors,
    const std::vector<std::vector<RelativePose>> *in_relatives, const std::vector<std::vector<uint8_t>> *obs_masks) {
  const int B = static_cast<int>(solvers.size());
  if (cov_poses != nullptr) cov_poses->assign(static_cast<size_t>(B), std::vector<Eigen::Matrix<double, 6, 6>>());
  if (cov_points != nullptr) cov_points->assign(static_cast<size_t>(B), std::vector<Eigen::Matrix<double, 3, 3>>());
  if (B == 0) return true;
  if (cov_poses == nullptr) throw std::runtime_error("ComputeCovarianceBatch: null output for the pose blocks");
  BatchArrays a;
  PackBatch(solvers, "ComputeCovarianceBatch", false, &a);
  PriorArrays pa;
  PackPriors(solvers, "ComputeCovarianceBatch", in_priors, sigma_pixel, &pa);
  RelativeArrays ra;
  PackRelatives(solvers, "ComputeCovarianceBatch", in_relatives, sigma_pixel, &ra);
  std::vector<uint8_t> mask;
  const bool masked = PackMasks(a, "ComputeCovarianceBatch", obs_masks, &mask);
  std::vector<double> cp(36 * a.pose_fixed.size()), cq(cov_points ? 9 * a.point_fixed.size() : 0);
  std::vector<ba_batch_cov_result> res(static_cast<size_t>(B));
  const Options defaults;
  ba_handle *h = nullptr;
  ba_batch *batch = nullptr;
  int rc = CreateBatch(a, solvers[0]->device_id_, &h, &batch);
  if (rc == 0) rc = SetPriors(batch, pa);
  if (rc == 0) rc = SetRelatives(batch, ra);
  if (rc == 0 && masked) rc = ba_batch_set_obs_mask(batch, mask.data());
  if (rc == 0)
    rc = ba_batch_covariance(batch, static_cast<double>(defaults.outlier_handle.threshold_huber_loss), cp.data(),
                             cov_points ? cq.data() : nullptr, res.data());
  const std::string err = rc ? ba_last_error() : "";
  ba_batch_destroy(batch);
  ba_destroy(h);
  if (rc) throw std::runtime_error("ComputeCovarianceBatch failed: " + err);
  // scaled units, unit pixel noise -> the caller's units (see ComputeCovariance)
  bool all_good = true;
  for (int b = 0; b < B; ++b) {
    const FullBundleAdjustmentSolver *s = solvers[b];
    const double s2 = sigma_pixel * sigma_pixel;
    const double k_pose = s2 * static_cast<double>(s->scaler_) * static_cast<double>(s->scaler_);
    all_good = all_good && res[b].status == 0 && res[b].dropped_pivots == 0;
    auto &out_p = (*cov_poses)[b];
    out_p.resize(static_cast<size_t>(a.pose_off[b + 1] - a.pose_off[b]));
    for (size_t k = 0; k < out_p.size(); ++k) {
      const double *src = &cp[36 * (static_cast<size_t>(a.pose_off[b]) + k)];
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
          const double dr = r < 3 ? static_cast<double>(s->inverse_scaler_) : 1.0;
          const double dc = c < 3 ? static_cast<double>(s->inverse_scaler_) : 1.0;
          out_p[k](r, c) = k_pose * (dr * src[6 * r + c] * dc);
        }
    }
    if (cov_points == nullptr) continue;
    auto &out_q = (*cov_points)[b];
    out_q.resize(static_cast<size_t>(a.pt_off[b + 1] - a.pt_off[b]));
    for (size_t k = 0; k < out_q.size(); ++k) {
      const double *src = &cq[9 * (static_cast<size_t>(a.pt_off[b]) + k)];
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out_q[k](r, c) = s2 * src[3 * r + c];
    }
  }
  return all_good;
}

bool FullBundleAdjustmentSolver::MarginalizeBatch(const std::vector<FullBundleAdjustmentSolver *> &solvers,
                                                  const std::vector<std::vector<_BA_Pose *>> &marg_poses,
                                                  double sigma_pixel, std::vector<MarginalPrior> *priors,
                                                  const std::vector<PosePrior> *in_priors,
                                                  const std::vector<std::vector<RelativePose>> *in_relatives,
                                                  const std::vector<std::vector<uint8_t>> *obs_masks) {
  const int B = static_cast<int>(solvers.size());
  if (priors == nullptr) throw std::runtime_error("MarginalizeBatch: null output");
  priors->assign(static_cast<size_t>(B), MarginalPrior());
  if (marg_poses.size() != solvers.size()) throw std::runtime_error("MarginalizeBatch: one list of poses per solver");
  if (B == 0) return true;
  BatchArrays a;
  PackBatch(solvers, "MarginalizeBatch", false, &a);
  PriorArrays pa;
  PackPriors(solvers, "MarginalizeBatch", in_priors, sigma_pixel, &pa);
  RelativeArrays ra;
  PackRelatives(solvers, "MarginalizeBatch", in_relatives, sigma_pixel, &ra);
  std::vector<uint8_t> mask;
  const bool masked = PackMasks(a, "MarginalizeBatch", obs_masks, &mask);
  std::vector<uint8_t> left(ra.set ? ra.j.size() : 0, 0);
  std::vector<uint8_t> mark(a.pose_fixed.size(), 0), marg_pt(a.point_fixed.size(), 0);
  for (int b = 0; b < B; ++b)
    for (_BA_Pose *pose : marg_poses[b]) {
      const auto it = solvers[b]->pose_index_.find(pose);
      if (it == solvers[b]->pose_index_.end())
        throw std::runtime_error("MarginalizeBatch: there is no pointer in the BA pose pool.");
      mark[static_cast<size_t>(a.pose_off[b] + it->second)] = 1;
    }
  std::vector<int64_t> H_off(static_cast<size_t>(B) + 1), b_off(static_cast<size_t>(B) + 1);
  std::vector<double> H, bv;
  std::vector<ba_batch_marg_result> res(static_cast<size_t>(B));
  const Options defaults;
  ba_handle *h = nullptr;
  ba_batch *batch = nullptr;
  int rc = CreateBatch(a, solvers[0]->device_id_, &h, &batch);
  if (rc == 0) rc = SetPriors(batch, pa);
  if (rc == 0) rc = SetRelatives(batch, ra);
  if (rc == 0 && masked) rc = ba_batch_set_obs_mask(batch, mask.data());
  if (rc == 0 && ra.set) rc = ba_batch_relative_marg_plan(batch, mark.data(), left.data());
  if (rc == 0) rc = ba_batch_marg_layout(batch, mark.data(), H_off.data(), b_off.data());
  if (rc == 0) {
    H.resize(static_cast<size_t>(H_off[B]));
    bv.resize(static_cast<size_t>(b_off[B]));
    rc = ba_batch_marginalize(batch, static_cast<double>(defaults.outlier_handle.threshold_huber_loss), mark.data(),
                              H.empty() ? nullptr : H.data(), bv.empty() ? nullptr : bv.data(), marg_pt.data(),
                              res.data());
  }
  const std::string err = rc ? ba_last_error() : "";
  ba_batch_destroy(batch);
  ba_destroy(h);
  if (rc) throw std::runtime_error("MarginalizeBatch failed: " + err);
  // scaled units, unit pixel noise -> the caller's units: the inverse of ComputeCovariance's
  bool all_good = true;
  for (int b = 0; b < B; ++b) {
    const FullBundleAdjustmentSolver *s = solvers[b];
    MarginalPrior &out = (*priors)[b];
    out.status = res[b].status;
    out.dropped_pivots = res[b].dropped_pivots;
    all_good = all_good && res[b].status == 0 && res[b].dropped_pivots == 0;
    for (size_t p = 0; p < s->poses_.size(); ++p)
      if (!a.pose_fixed[a.pose_off[b] + p] && !mark[a.pose_off[b] + p]) out.kept_poses.push_back(s->poses_[p]);
    for (size_t q = 0; q < s->points_.size(); ++q)
      if (marg_pt[a.pt_off[b] + q]) out.marginalized_points.push_back(s->points_[q]);
    if (ra.set) out.relatives_left.assign(left.begin() + ra.off[b], left.begin() + ra.off[b + 1]);
    out.dim = static_cast<int>(b_off[b + 1] - b_off[b]);
    const double w = 1.0 / (sigma_pixel * sigma_pixel * static_cast<double>(s->scaler_) * static_cast<double>(s->scaler_));
    const auto di = [s](int r) { return r % 6 < 3 ? static_cast<double>(s->scaler_) : 1.0; };
    out.H.resize(static_cast<size_t>(out.dim) * out.dim);
    out.b.resize(static_cast<size_t>(out.dim));
    for (int r = 0; r < out.dim; ++r) {
      for (int c = 0; c < out.dim; ++c)
        out.H[static_cast<size_t>(r) * out.dim + c] =
            w * (di(r) * H[static_cast<size_t>(H_off[b]) + static_cast<size_t>(r) * out.dim + c] * di(c));
      out.b[r] = w * (di(r) * bv[static_cast<size_t>(b_off[b]) + r]);
    }
  }
  return all_good;
}

}  // namespace analytic_solver
}  // namespace visual_navigation
