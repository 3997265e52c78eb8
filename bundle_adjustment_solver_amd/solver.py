"""Python mirror of the reference's solver interface over the HIP C ABI.

Mirrors (names, argument meaning, error behaviour):
  * FullBundleAdjustmentSolver   reference core/full_bundle_adjustment_solver.h:127-146
  * PoseOnlyBundleAdjustmentSolver.Solve_{Monocular,Stereo}_{6Dof,Planar3Dof}
                                 reference core/pose_only_bundle_adjustment_solver.h:25-67
  * Options / Summary / OptimizationInfo / IterationStatus / SolverType
                                 reference core/solver_option_and_summary.h:25-93
Everything numerical happens in libba_hip.so (include/ba_hip.h); this module
only does what the reference's facade does on the host: pointer(identity)->
index maps, the 0.01 scaling, pose inversion and the final write-back.
"""
import collections
import ctypes as C
import enum
import sys
import time

import numpy as np

from . import _lib
from ._lib import (BaIterInfo, BaOptions, BaPointResult, BaPoIter, BaPoResult,
                   check)

SCALER = 0.01          # reference core/full_bundle_adjustment_solver.cpp:38
INVERSE_SCALER = 1.0 / SCALER


class SolverType(enum.IntEnum):
    UNDEFINED = -1
    GRADIENT_DESCENT = 0
    GAUSS_NEWTON = 1
    LEVENBERG_MARQUARDT = 2


class IterationStatus(enum.IntEnum):
    UNDEFINED = -1
    UPDATE = 0
    UPDATE_TRUST_MORE = 1
    SKIPPED = 2


class OptimizationInfo:
    def __init__(self):
        self.cost = -1.0
        self.cost_change = -1.0
        self.average_reprojection_error = -1.0
        self.abs_gradient = -1.0
        self.abs_step = -1.0
        self.damping_term = -1.0
        self.iter_time = -1.0
        self.iteration_status = IterationStatus.UNDEFINED
        # extras (not in the reference): trust-region internals
        self.rho = float("nan")
        self.model_change = float("nan")
        self.trial_cost = float("nan")


class _Handle:
    pass


class Options:
    """reference core/solver_option_and_summary.h:47-71 (float fields)."""

    def __init__(self):
        self.solver_type = SolverType.GAUSS_NEWTON  # ignored by full BA (Q10)
        self.convergence_handle = _Handle()
        self.convergence_handle.threshold_step_size = 1e-5
        self.convergence_handle.threshold_cost_change = 1e-5
        self.outlier_handle = _Handle()
        self.outlier_handle.threshold_huber_loss = 1.0
        self.outlier_handle.threshold_outlier_rejection = 2.0
        self.iteration_handle = _Handle()
        self.iteration_handle.max_num_iterations = 50
        self.trust_region_handle = _Handle()
        self.trust_region_handle.initial_lambda = 100.0
        self.trust_region_handle.decrease_ratio_lambda = 0.33
        self.trust_region_handle.increase_ratio_lambda = 3.0

    def to_c(self):
        o = BaOptions()
        o.threshold_step_size = self.convergence_handle.threshold_step_size
        o.threshold_cost_change = self.convergence_handle.threshold_cost_change
        o.threshold_huber_loss = self.outlier_handle.threshold_huber_loss
        o.threshold_outlier_rejection = \
            self.outlier_handle.threshold_outlier_rejection
        o.max_num_iterations = int(self.iteration_handle.max_num_iterations)
        o.initial_lambda = self.trust_region_handle.initial_lambda
        o.decrease_ratio_lambda = \
            self.trust_region_handle.decrease_ratio_lambda
        o.increase_ratio_lambda = \
            self.trust_region_handle.increase_ratio_lambda
        return o


class CullOptions:
    """The two-stage local BA of SolveBatch(..., cull=...): `first` are the Options of the
    first solve; an observation is then switched off when its squared reprojection error
    exceeds chi2 * sigma_pixel^2 pixels^2 (5.991: 95 % of a chi-square of two degrees of
    freedom) or, with cull_behind, when it lies behind its camera."""

    def __init__(self, first=None, chi2=5.991, cull_behind=True):
        self.first = Options() if first is None else first
        self.chi2 = chi2
        self.cull_behind = cull_behind

    def e2_max_scaled(self, sigma_pixel=1.0):
        """the threshold in the library's units (pixels x SCALER, squared)"""
        return float(self.chi2) * float(sigma_pixel) ** 2 * SCALER * SCALER


def _yellow(s):
    return "\033[0;33m" + s + "\033[0m"


def _green(s):
    return "\033[0;32m" + s + "\033[0m"


class Summary:
    """reference core/solver_option_and_summary.h:74-93, .cpp:8-84."""

    def __init__(self):
        self.optimization_info_list_ = []
        self.max_iteration_ = 0
        self.total_time_in_millisecond_ = 0.0
        self.threshold_step_size_ = 0.0
        self.threshold_cost_change_ = 0.0
        self.convergence_status_ = False

    def GetTotalTimeInSecond(self):
        return self.total_time_in_millisecond_ * 0.001

    def BriefReport(self):
        lines = ["itr   total_cost   avg.reproj.  cost_change  |step|   "
                 "|gradient|  damp_term  itr_time[ms] itr_stat"]
        for it, info in enumerate(self.optimization_info_list_):
            row = "%3d  %.6e    %.2e    %.2e   %.2e   %.2e    %.2e   %.2e" % (
                it, info.cost, info.average_reprojection_error,
                info.cost_change, info.abs_step, info.abs_gradient,
                info.damping_term, info.iter_time)
            if info.iteration_status == IterationStatus.UPDATE:
                row += "     UPDATE"
            elif info.iteration_status == IterationStatus.SKIPPED:
                row += "     " + _yellow(" SKIP ")
            elif info.iteration_status == IterationStatus.UPDATE_TRUST_MORE:
                row += "     " + _green("UPDATE")
            else:
                row += "     "
            lines.append(row)
        n = len(self.optimization_info_list_)
        lines.append("Analytic Solver Report:")
        lines.append("  Iterations      : %d" % n)
        lines.append("  Total time      : %.5g [second]" %
                     (self.total_time_in_millisecond_ * 0.001))
        if n:  # the reference dereferences front()/back() unconditionally
            first, last = (self.optimization_info_list_[0],
                           self.optimization_info_list_[-1])
            lines.append("  Initial cost    : %.5g" % first.cost)
            lines.append("  Final cost      : %.5g" % last.cost)
            lines.append("  Initial reproj. : %.5g [pixel]" %
                         first.average_reprojection_error)
            lines.append("  Final reproj.   : %.5g [pixel]" %
                         last.average_reprojection_error)
        lines.append(", Termination     : " +
                     (_green("CONVERGENCE") if self.convergence_status_
                      else _yellow("NO_CONVERGENCE")))
        if self.max_iteration_ == n:
            lines.append(_yellow(" WARNIING: MAX ITERATION is reached ! The "
                                 "solution could be local minima."))
        return "\n".join(lines) + "\n"


class Camera:
    """_BA_Camera, reference core/full_bundle_adjustment_solver.h:92-107."""

    def __init__(self, fx=0.0, fy=0.0, cx=0.0, cy=0.0, pose_this_to_cam0=None):
        self.fx, self.fy, self.cx, self.cy = fx, fy, cx, cy
        self.pose_this_to_cam0 = (np.eye(4) if pose_this_to_cam0 is None
                                  else np.array(pose_this_to_cam0, float))


def rigid_inverse(T):
    """Isometry inverse (R^T, -R^T t) as Eigen's Transform<..., Isometry>
    (SURVEY Q11); works on (..., 4, 4)."""
    T = np.asarray(T, dtype=np.float64)
    R = T[..., :3, :3]
    t = T[..., :3, 3]
    out = np.zeros_like(T)
    Rt = np.swapaxes(R, -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -np.einsum("...ij,...j->...i", Rt, t)
    out[..., 3, 3] = 1.0
    return out


def _T44_to_12(T):
    T = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)
    return np.concatenate([T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]], axis=1)


def _T12_to_44(T12):
    T12 = np.asarray(T12, dtype=np.float64).reshape(-1, 12)
    out = np.zeros((T12.shape[0], 4, 4))
    out[:, :3, :3] = T12[:, :9].reshape(-1, 3, 3)
    out[:, :3, 3] = T12[:, 9:]
    out[:, 3, 3] = 1.0
    return out


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def covariance_to_user_units(cov_pose, cov_pt, sigma_px):
    """Blocks of BaProblem.covariance (scaled units, unit pixel noise) -> covariances
    in the caller's units for an isotropic pixel noise of sigma_px (numpy only).

    The facade scales lengths and pixels by SCALER = 0.01.  A residual of r pixels
    is 0.01 r scaled, so a noise of sigma_px is 0.01 sigma_px there and the scaled
    covariance is (1e-4 sigma_px^2) Sigma_s.  The rotation part omega of the pose
    tangent xi = [v; omega] (T_jw <- exp(xi) T_jw, world-to-body,
    left-multiplicative) has no unit, v is a length: xi_user = D xi_scaled with
    D = diag(100 I3, I3); a point is a length: X_user = 100 X_scaled.  Hence
        Cov_pose  = sigma_px^2 * 1e-4 * D Sigma_s D
        Cov_point = sigma_px^2 * 1e-4 * 1e4 * Sigma_s = sigma_px^2 * Sigma_s."""
    cov_pose = np.asarray(cov_pose, np.float64).reshape(-1, 6, 6)
    cov_pt = np.asarray(cov_pt, np.float64).reshape(-1, 3, 3)
    s2 = float(sigma_px) ** 2
    d = np.r_[np.full(3, INVERSE_SCALER), np.ones(3)]
    return (s2 * SCALER * SCALER) * (d[None, :, None] * cov_pose * d[None, None, :]), s2 * cov_pt


def marginal_to_user_units(H, b, sigma_px):
    """A prior of BaBatch.marginalize (scaled units, unit pixel noise) -> information
    matrix and vector in the caller's units for an isotropic pixel noise of sigma_px
    (numpy only): the inverse of covariance_to_user_units.  With xi_user = D xi_scaled
    per pose, D = diag(100 I3, I3), and a noise of 0.01 sigma_px in scaled pixels,
        H_u = D^-1 H D^-1 / (1e-4 sigma_px^2),    b_u = D^-1 b / (1e-4 sigma_px^2),
    so that H_u delta_u = b_u is the same step and 1/2 d^T H_u d - b_u^T d the energy
    in units of that noise."""
    H = np.asarray(H, np.float64)
    b = np.asarray(b, np.float64)
    K = b.shape[0] // 6
    di = np.tile(np.r_[np.full(3, SCALER), np.ones(3)], K)
    w = 1.0 / (float(sigma_px) ** 2 * SCALER * SCALER)
    return w * (di[:, None] * H.reshape(6 * K, 6 * K) * di[None, :]), w * (di * b)


def prior_to_scaled_units(H_u, b_u, c_u, sigma_px):
    """A prior in the caller's units (what MarginalizeBatch returns, plus its constant)
    -> (H, b, c) in scaled units with unit pixel noise, the input of BaBatch.set_prior:
    the exact inverse of marginal_to_user_units.  With D^-1 = diag(0.01 I3, I3) per pose and
    the weight w = 1 / (1e-4 sigma_px^2) of that function,
        H = D H_u D / w,    b = D b_u / w,    c = c_u / w
    (c is an energy like d^T H_u d: it carries the weight and no D)."""
    H_u = np.asarray(H_u, np.float64)
    b_u = np.asarray(b_u, np.float64)
    K = b_u.shape[0] // 6
    d = np.tile(np.r_[np.full(3, INVERSE_SCALER), np.ones(3)], K)
    w = 1.0 / (float(sigma_px) ** 2 * SCALER * SCALER)
    return (d[:, None] * H_u.reshape(6 * K, 6 * K) * d[None, :]) / w, (d * b_u) / w, float(c_u) / w


PRIOR_RCOND = 1e-12


def prior_constant(H, b, rcond=PRIOR_RCOND):
    """c = b^T H^+ b of a prior (numpy, symmetric eigendecomposition of (H + H^T) / 2):
    with it the prior's cost term sqrt(d^T H d - 2 b^T d + c) is zero at the prior's own
    minimum.  H^+ inverts the eigenvalues above rcond * (the largest eigenvalue) and drops
    the others (the gauge null space of a marginal; default rcond = 1e-12, four decades
    above the rounding of the eigenvalues)."""
    H = np.asarray(H, np.float64)
    b = np.asarray(b, np.float64).reshape(-1)
    if b.size == 0:
        return 0.0
    w, V = np.linalg.eigh(0.5 * (H + H.T))
    keep = w > rcond * max(w.max(), 0.0)
    y = V[:, keep].T @ b
    return float(np.sum(y * y / w[keep]))


def se3_log(T12):
    """The device se3_log (csrc/ba_device_fn.h) restated in numpy: T12 = [R row-major, t]
    -> x = [v; omega] with se3_exp(x) = T; defined for a rotation angle below pi."""
    T12 = np.asarray(T12, np.float64).reshape(12)
    R, t = T12[:9].reshape(3, 3), T12[9:]
    a = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    sn = 0.5 * np.sqrt(a @ a)
    cs = 0.5 * (np.trace(R) - 1.0)
    theta = np.arctan2(sn, cs)
    if theta < 1e-7:
        f, k = 0.5, 1.0 / 12.0
    else:
        hf = 0.5 * theta
        f = theta / (2.0 * sn)
        k = (1.0 - hf * np.cos(hf) / np.sin(hf)) / (theta * theta)
    w = f * a
    c = np.cross(w, t)
    return np.r_[t - 0.5 * c + k * np.cross(w, c), w]


def prior_delta(T12, T_lin12):
    """delta = se3_log(T T_lin^-1), the tangent the prior of BaBatch.set_prior acts on."""
    T = _T12_to_44(T12)[0]
    L = _T12_to_44(T_lin12)[0]
    return se3_log(_T44_to_12(T @ rigid_inverse(L))[0])


def relative_residual(T_j12, T_k12, Z12):
    """r = se3_log(T_j T_k^-1 Z^-1), the residual of a relative-pose factor of
    BaBatch.set_relative: prior_delta with T_lin = Z T_k."""
    Tj = _T12_to_44(T_j12)[0]
    Tk = _T12_to_44(T_k12)[0]
    Z = _T12_to_44(Z12)[0]
    return se3_log(_T44_to_12(Tj @ rigid_inverse(Tk) @ rigid_inverse(Z))[0])


def relative_adjoint(T_j12, T_k12):
    """Ad(E) of E = T_j T_k^-1 = [R, t]: [[R, [t]x R], [0, R]] (6, 6), the device's rel_Ad
    (csrc/ba_rel_fn.h) in numpy; the factor's Jacobian with respect to xi_k is -Ad(E)."""
    E = _T12_to_44(T_j12)[0] @ rigid_inverse(_T12_to_44(T_k12)[0])
    R, t = E[:3, :3], E[:3, 3]
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = Ad[3:, 3:] = R
    Ad[:3, 3:] = tx @ R
    return Ad


def relative_covariance(T_j12, T_k12, S_jj, S_jk, S_kk):
    """Sigma_E of BaPoseGraph.covariance on the host (numpy only): E = T_j T_k^-1 moves to first
    order by xi_E = xi_j - Ad(E) xi_k, hence
        Sigma_E = S_jj - S_jk Ad^T - Ad S_jk^T + Ad S_kk Ad^T.
    A fixed pose has zero blocks: with j fixed this is Ad S_kk Ad^T, with k fixed S_jj."""
    Ad = relative_adjoint(T_j12, T_k12)
    S_jj, S_jk, S_kk = (np.asarray(S, np.float64).reshape(6, 6) for S in (S_jj, S_jk, S_kk))
    return S_jj - S_jk @ Ad.T - Ad @ S_jk.T + Ad @ S_kk @ Ad.T


class BaProblem:
    """Thin numpy wrapper over one ba_handle, in the solver's SCALED units.

    This is the level the parity tests drive: set_* / finalize / stage_* /
    get_* map one-to-one onto the C ABI.
    """

    def __init__(self, device=0):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.ba_create(C.byref(h), device), "ba_create")
        self.h = h
        self.device = device
        self._keep = []
        self.n_pose = self.n_pt = 0
        self.N = self.M = 0
        self.M_global = 0

    def close(self):
        if self.h:
            self.lib.ba_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- construction --
    def set_cameras(self, intr4, T_cj12):
        intr4 = np.ascontiguousarray(intr4, np.float64).reshape(-1, 4)
        T = np.ascontiguousarray(T_cj12, np.float64).reshape(-1, 12)
        check(self.lib.ba_set_cameras(self.h, intr4.shape[0], _dp(intr4),
                                      _dp(T)), "ba_set_cameras")

    def set_poses(self, T_jw12, fixed):
        T = np.ascontiguousarray(T_jw12, np.float64).reshape(-1, 12)
        f = np.ascontiguousarray(fixed, np.uint8)
        self.n_pose = T.shape[0]
        self.pose_fixed = f.copy()
        check(self.lib.ba_set_poses(self.h, T.shape[0], _dp(T), _up(f)),
              "ba_set_poses")

    def set_points(self, X3, fixed):
        X = np.ascontiguousarray(X3, np.float64).reshape(-1, 3)
        f = np.ascontiguousarray(fixed, np.uint8)
        self.n_pt = X.shape[0]
        self.pt_fixed = f.copy()
        check(self.lib.ba_set_points(self.h, X.shape[0], _dp(X), _up(f)),
              "ba_set_points")

    def set_observations(self, cam, pose, pt, uv):
        cam = np.ascontiguousarray(cam, np.int32)
        pose = np.ascontiguousarray(pose, np.int32)
        pt = np.ascontiguousarray(pt, np.int32)
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        check(self.lib.ba_set_observations(self.h, cam.shape[0], _ip(cam),
                                           _ip(pose), _ip(pt), _dp(uv)),
              "ba_set_observations")

    def set_shard(self, rank, world):
        check(self.lib.ba_set_shard(self.h, rank, world), "ba_set_shard")

    def set_stream(self, stream_ptr):
        check(self.lib.ba_set_stream(self.h, C.c_void_p(stream_ptr)),
              "ba_set_stream")

    def finalize(self):
        check(self.lib.ba_finalize(self.h), "ba_finalize")
        self.N = self.lib.ba_num_opt_poses(self.h)
        self.M = self.lib.ba_num_opt_points(self.h)
        self.M_global = int(np.sum(self.pt_fixed == 0))
        self.P = self.lib.ba_num_pairs(self.h)

    def update_values(self, T_jw12=None, X3=None):
        """New parameter values for the finalized structure (no re-planning)."""
        T = None if T_jw12 is None else np.ascontiguousarray(T_jw12, np.float64).reshape(-1, 12)
        X = None if X3 is None else np.ascontiguousarray(X3, np.float64).reshape(-1, 3)
        if T is not None and T.shape[0] != self.n_pose or X is not None and X.shape[0] != self.n_pt:
            raise ValueError("update_values: the structure is fixed (same number of poses / points)")
        check(self.lib.ba_update_values(self.h, None if T is None else _dp(T),
                                        None if X is None else _dp(X)), "ba_update_values")

    def set_relative(self, rels):
        """Relative-pose factors of the handle (ba_set_relative; scaled units), before
        finalize.  rels: None (clears) or a dict j (F,), k (F,) user pose indices, Z (F, 12)
        the measurement of T_j T_k^-1, Omega (F, 6, 6) of which the lower triangle counts."""
        refuse_robust("set_relative", rels)
        if rels is None or len(np.asarray(rels["j"]).reshape(-1)) == 0:
            check(self.lib.ba_set_relative(self.h, 0, None, None, None, None), "ba_set_relative")
            self._n_rel = 0
            return
        j = np.ascontiguousarray(rels["j"], np.int32).reshape(-1)
        k = np.ascontiguousarray(rels["k"], np.int32).reshape(-1)
        Z = np.ascontiguousarray(rels["Z"], np.float64).reshape(-1, 12)
        Om = np.ascontiguousarray(rels["Omega"], np.float64).reshape(-1, 36)
        if not (len(k) == len(j) and Z.shape[0] == len(j) and Om.shape[0] == len(j)):
            raise ValueError("set_relative: needs j (F,), k (F,), Z (F, 12), Omega (F, 6, 6)")
        check(self.lib.ba_set_relative(self.h, len(j), _ip(j), _ip(k), _dp(Z), _dp(Om)), "ba_set_relative")
        self._n_rel = len(j)

    def update_relative(self, Z, Omega):
        """New Z (F, 12) and Omega (F, 6, 6) for the same pairs on the finalized handle
        (ba_update_relative: no re-planning)."""
        Z = np.ascontiguousarray(Z, np.float64).reshape(-1, 12)
        Om = np.ascontiguousarray(Omega, np.float64).reshape(-1, 36)
        n = getattr(self, "_n_rel", 0)
        if Z.shape[0] != n or Om.shape[0] != n:
            raise ValueError("update_relative: one Z and one Omega per factor of set_relative (%d)" % n)
        check(self.lib.ba_update_relative(self.h, _dp(Z), _dp(Om)), "ba_update_relative")

    def relative_info(self):
        """-> dict: factors, blocks of S that carry a factor, blocks that exist only because
        of a factor, device bytes of the factor records and scratch (ba_relative_info)"""
        out = (C.c_int64 * 4)()
        check(self.lib.ba_relative_info(self.h, out), "ba_relative_info")
        return dict(factors=int(out[0]), blocks=int(out[1]), blocks_only=int(out[2]), bytes=int(out[3]))

    def set_allreduce(self, pyfunc):
        """pyfunc(which:int, dev_ptr:int, n_doubles:int, stream:int) -> int"""
        def _cb(user, which, ptr, n, stream):
            try:
                return int(pyfunc(which, ptr or 0, n, stream or 0) or 0)
            except Exception as e:  # never let an exception cross the ABI
                sys.stderr.write("all-reduce hook failed: %r\n" % (e,))
                return 1
        cb = _lib.ALLREDUCE_FN(_cb)
        self._keep.append(cb)
        check(self.lib.ba_set_allreduce(self.h, cb, None), "ba_set_allreduce")

    def set_allreduce_native(self, fn_ptr, user_ptr):
        """Register a C function (ba_allreduce_fn, e.g. ba_rccl_allreduce_hook)
        with its user pointer: no Python inside the LM loop."""
        fn = C.cast(fn_ptr, _lib.ALLREDUCE_FN)
        self._keep.append(fn)
        check(self.lib.ba_set_allreduce(self.h, fn, C.c_void_p(user_ptr)),
              "ba_set_allreduce")

    def gather_points(self):
        """Final exchange of a sharded Solve (reference :1018-1022 writes back
        every point): afterwards get_points() returns all points on every rank."""
        check(self.lib.ba_gather_points(self.h), "ba_gather_points")

    def reduce_buffer_size(self, which):
        return int(self.lib.ba_reduce_buffer_size(self.h, which))

    def bind_reduce_buffer(self, which, dev_ptr, n):
        check(self.lib.ba_bind_reduce_buffer(self.h, which,
                                             C.c_void_p(dev_ptr), n),
              "ba_bind_reduce_buffer")

    # -- LM loop --
    def solve(self, opt, cap=None):
        cap = cap or max(1, opt.max_num_iterations)
        rows = (BaIterInfo * cap)()
        n = C.c_int(0)
        conv = C.c_int(0)
        check(self.lib.ba_solve(self.h, C.byref(opt), rows, cap, C.byref(n),
                                C.byref(conv)), "ba_solve")
        return [rows[i] for i in range(min(n.value, cap))], bool(conv.value)

    def lm_begin(self, opt):
        check(self.lib.ba_lm_begin(self.h, C.byref(opt)), "ba_lm_begin")

    def lm_iterate(self, n):
        check(self.lib.ba_lm_iterate(self.h, n), "ba_lm_iterate")

    def lm_sync(self, cap=0):
        rows = (BaIterInfo * max(cap, 1))()
        n = C.c_int(0)
        conv = C.c_int(0)
        rc = check(self.lib.ba_lm_sync(self.h, rows, cap, C.byref(n),
                                       C.byref(conv)), "ba_lm_sync")
        return ([rows[i] for i in range(min(n.value, cap))], n.value,
                bool(conv.value), bool(rc))

    # -- gradient descent (reference ..._refactor.cpp:1075-1367) --
    def solve_gd(self, opt, cap=None):
        cap = cap or max(1, opt.max_num_iterations)
        rows = (BaIterInfo * cap)()
        n = C.c_int(0)
        conv = C.c_int(0)
        check(self.lib.ba_solve_gd(self.h, C.byref(opt), rows, cap, C.byref(n),
                                   C.byref(conv)), "ba_solve_gd")
        return [rows[i] for i in range(min(n.value, cap))], bool(conv.value)

    def gd_begin(self, opt):
        check(self.lib.ba_gd_begin(self.h, C.byref(opt)), "ba_gd_begin")

    def gd_iterate(self, n):
        check(self.lib.ba_gd_iterate(self.h, n), "ba_gd_iterate")

    def gd_sync(self, cap=0):
        rows = (BaIterInfo * max(cap, 1))()
        n = C.c_int(0)
        conv = C.c_int(0)
        rc = check(self.lib.ba_gd_sync(self.h, rows, cap, C.byref(n),
                                       C.byref(conv)), "ba_gd_sync")
        return ([rows[i] for i in range(min(n.value, cap))], n.value,
                bool(conv.value), bool(rc))

    def gd_gradient(self):
        """Unclipped (a, b) at the current parameters: a (N, 6) in opt-pose
        order, b (M, 3) in opt-point order (the layout of get_A / get_C)."""
        a = np.zeros((self.N, 6))
        b = np.zeros((self.M_global, 3))
        check(self.lib.ba_gd_get_gradient(self.h, _dp(a), _dp(b)),
              "ba_gd_get_gradient")
        return a, b

    # -- stages --
    def stage_cost(self):
        v = C.c_double(0)
        check(self.lib.ba_stage_cost(self.h, C.byref(v)), "ba_stage_cost")
        return v.value

    def stage_linearize(self, lam, huber):
        check(self.lib.ba_stage_linearize(self.h, lam, huber),
              "ba_stage_linearize")

    def stage_schur(self):
        check(self.lib.ba_stage_schur(self.h), "ba_stage_schur")

    def stage_solve_reduced(self):
        check(self.lib.ba_stage_solve_reduced(self.h),
              "ba_stage_solve_reduced")

    def stage_backsub_update(self):
        check(self.lib.ba_stage_backsub_update(self.h),
              "ba_stage_backsub_update")

    def stage_scalars(self):
        a, b, c, d = (C.c_double(0) for _ in range(4))
        check(self.lib.ba_stage_scalars(self.h, C.byref(a), C.byref(b),
                                        C.byref(c), C.byref(d)),
              "ba_stage_scalars")
        return a.value, b.value, c.value, d.value

    def stage_commit(self, accept):
        check(self.lib.ba_stage_commit(self.h, int(bool(accept))),
              "ba_stage_commit")

    def enable_stage_timing(self, on=True):
        check(self.lib.ba_enable_stage_timing(self.h, int(on)),
              "ba_enable_stage_timing")

    def get_stage_ms(self, reset=True):
        out = np.zeros(8)
        check(self.lib.ba_get_stage_ms(self.h, _dp(out), int(reset)),
              "ba_get_stage_ms")
        return out

    # -- readers --
    def get_poses(self):
        out = np.zeros((self.n_pose, 12))
        check(self.lib.ba_get_poses(self.h, _dp(out)), "ba_get_poses")
        return out

    def get_points(self, into=None):
        out = np.zeros((self.n_pt, 3)) if into is None else into
        mask = np.zeros(self.n_pt, np.uint8)
        check(self.lib.ba_get_points(self.h, _dp(out), _up(mask)),
              "ba_get_points")
        return out, mask.astype(bool)

    def get_A(self):
        A = np.zeros((self.N, 6, 6))
        a = np.zeros((self.N, 6))
        check(self.lib.ba_get_A(self.h, _dp(A), _dp(a)), "ba_get_A")
        return A, a

    def get_C(self):
        Cm = np.zeros((self.M_global, 3, 3))
        b = np.zeros((self.M_global, 3))
        check(self.lib.ba_get_C(self.h, _dp(Cm), _dp(b)), "ba_get_C")
        return Cm, b

    def get_Cinv(self):
        Ci = np.zeros((self.M_global, 3, 3))
        cb = np.zeros((self.M_global, 3))
        check(self.lib.ba_get_Cinv(self.h, _dp(Ci), _dp(cb)), "ba_get_Cinv")
        return Ci, cb

    def get_pairs(self):
        P = int(self.P)
        pi = np.zeros(P, np.int32)
        pj = np.zeros(P, np.int32)
        W = np.zeros((P, 6, 3))
        check(self.lib.ba_get_pairs(self.h, _ip(pi), _ip(pj), _dp(W)),
              "ba_get_pairs")
        return pi, pj, W

    def get_S(self):
        n6 = 6 * self.N
        S = np.zeros((n6, n6))
        rhs = np.zeros(n6)
        check(self.lib.ba_get_S(self.h, _dp(S), _dp(rhs)), "ba_get_S")
        return S, rhs

    def get_xy(self):
        x = np.zeros((self.N, 6))
        y = np.zeros((self.M_global, 3))
        check(self.lib.ba_get_xy(self.h, _dp(x), _dp(y)), "ba_get_xy")
        return x, y

    def get_kernel_ms(self, reset=True):
        """{kernel name: (total ms, launches)} accumulated in timing mode."""
        n = self.lib.ba_kernel_count()
        ms = np.zeros(n)
        calls = np.zeros(n, np.int64)
        check(self.lib.ba_get_kernel_ms(
            self.h, _dp(ms), calls.ctypes.data_as(C.POINTER(C.c_int64)),
            int(reset)), "ba_get_kernel_ms")
        return {self.lib.ba_kernel_name(k).decode(): (float(ms[k]), int(calls[k]))
                for k in range(n)}

    def get_dense_info(self):
        out = np.zeros(4)
        check(self.lib.ba_get_dense_info(self.h, _dp(out)),
              "ba_get_dense_info")
        return dict(fill=out[0], flops=out[1], levels=int(out[2]),
                    npad=int(out[3]))

    def get_schur_info(self):
        """How the Schur complement is accumulated: covisibility-group workgroups
        (32- / 64-wide tiles), landmarks they cover, super-runs for the rest."""
        v = (C.c_int64 * 8)()
        check(self.lib.ba_get_schur_info(self.h, v), "ba_get_schur_info")
        return dict(groups32=int(v[0]), groups64=int(v[1]), grouped_landmarks=int(v[2]),
                    super_runs=int(v[3]), grouped_pairs=int(v[4]), grouped_triples=int(v[5]),
                    group_mfma=int(v[6]), list_triples=int(v[7]))

    def get_lin_info(self):
        """How the shard is linearised: pieces of the covisibility-group kernel
        (landmark and pose side in one pass), the observations they cover, chunks left
        to the chunk kernel, observations on the pose-major list."""
        v = (C.c_int64 * 4)()
        check(self.lib.ba_get_lin_info(self.h, v), "ba_get_lin_info")
        return dict(group_pieces=int(v[0]), group_observations=int(v[1]), chunks=int(v[2]),
                    pose_major_observations=int(v[3]))

    def get_pair_record_info(self):
        """Pair records of this shard: how many are kept as the 64-byte record {G, w}
        (the pairs of the covisibility groups) and how many pairs there are."""
        v = (C.c_int64 * 2)()
        check(self.lib.ba_get_pair_record_info(self.h, v), "ba_get_pair_record_info")
        return dict(slim_pairs=int(v[0]), pairs=int(v[1]))

    def get_pair_form(self):
        """Record form of the grouped pairs: 0 = 96-byte, 1 = slim {G, w}, 2 = from the
        observation (no record in the iteration)."""
        f = self.lib.ba_get_pair_form(self.h)
        if f < 0:
            check(f, "ba_get_pair_form")
        return int(f)

    def get_slim_records(self):
        """The slim records of the grouped pairs as the device holds them (form 2: filled on
        demand), with pose, landmark, camera and uv of each pair's last writer."""
        n = self.get_pair_record_info()["slim_pairs"]
        pose, lm, cam = (np.zeros(n, np.int32) for _ in range(3))
        uv, rec = np.zeros((n, 2)), np.zeros((n, 8))
        check(self.lib.ba_get_slim_records(self.h, _ip(pose), _ip(lm), _ip(cam), _dp(uv), _dp(rec)),
              "ba_get_slim_records")
        return dict(pose=pose, lm=lm, cam=cam, uv=uv, rec=rec)

    def get_mask_info(self):
        """Superset (masked) covisibility groups of this shard."""
        v = (C.c_int64 * 4)()
        check(self.lib.ba_get_mask_info(self.h, v), "ba_get_mask_info")
        return dict(masked_pieces=int(v[0]), masked_landmarks=int(v[1]),
                    padded_observation_slots=int(v[2]), padded_pairs=int(v[3]))

    def get_dropped_pivots(self, reset=False):
        """Non-positive pivots met by the reduced-system Cholesky since lm_begin
        (see include/ba_hip.h: where it differs from the reference's pivoted
        LDLT)."""
        v = C.c_int64(0)
        check(self.lib.ba_get_dropped_pivots(self.h, C.byref(v), int(reset)),
              "ba_get_dropped_pivots")
        return int(v.value)

    def covariance(self, pose_sel, pt_sel, huber):
        """ba_covariance: blocks of the inverse of the solver's normal matrix
        [[A, W], [W^T, C]] at the current accepted values, lambda = 0 and the given
        Huber threshold, in SCALED units.  pose_sel / pt_sel: USER indices of
        optimisable poses / points (any order, repeats allowed, may be empty).
        Returns (cov_pose (n, 6, 6), cov_pt (n, 3, 3), dropped pivots of this
        call's factorisation).  Pose tangent: xi = [v; omega] of
        T_jw <- exp(xi) T_jw.  Afterwards the stage readers (get_A, get_S, ...)
        hold the lambda = 0 linearisation; poses, points and the LM state are
        untouched."""
        ps = np.ascontiguousarray(pose_sel, np.int32).reshape(-1)
        qs = np.ascontiguousarray(pt_sel, np.int32).reshape(-1)
        cp = np.zeros((ps.size, 6, 6))
        cq = np.zeros((qs.size, 3, 3))
        dropped = C.c_int64(0)
        check(self.lib.ba_covariance(self.h, float(huber), ps.size, _ip(ps) if ps.size else None,
                                     _dp(cp) if ps.size else None, qs.size,
                                     _ip(qs) if qs.size else None, _dp(cq) if qs.size else None,
                                     C.byref(dropped)), "ba_covariance")
        return cp, cq, int(dropped.value)

    def covariance_info(self):
        """Column batches of ba_covariance on this handle (BA_COV_BATCH overrides
        the width)."""
        v = (C.c_int64 * 4)()
        check(self.lib.ba_covariance_info(self.h, v), "ba_covariance_info")
        return dict(batch_cols=int(v[0]), cols_per_wave=int(v[1]), workspace_bytes=int(v[2]),
                    last_batches=int(v[3]))

    def dense_spd_solve(self, A, b):
        A = np.ascontiguousarray(A, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        n = A.shape[0]
        x = np.zeros(n)
        ms = C.c_double(0)
        check(self.lib.ba_dense_spd_solve(self.h, n, _dp(A), _dp(b), _dp(x),
                                          C.byref(ms)), "ba_dense_spd_solve")
        return x, ms.value

    def pose_only_mono6(self, X3, uv2, fx, fy, cx, cy, T12, mask, opt,
                        cap=None, want_debug=False):
        X = np.ascontiguousarray(X3, np.float32).reshape(-1, 3)
        uv = np.ascontiguousarray(uv2, np.float32).reshape(-1, 2)
        n = X.shape[0]
        T = np.ascontiguousarray(T12, np.float32).reshape(12).copy()
        m = np.ascontiguousarray(mask, np.uint8).copy()
        cap = cap or max(1, opt.max_num_iterations)
        rows = (BaPoIter * cap)()
        n_it = C.c_int(0)
        conv = C.c_int(0)
        dbg = np.zeros((cap, 12), np.float32) if want_debug else None
        rc = check(self.lib.ba_pose_only_mono6(
            self.h, _fp(X), _fp(uv), n, fx, fy, cx, cy, _fp(T), _up(m),
            C.byref(opt), rows, cap, C.byref(n_it), C.byref(conv),
            _fp(dbg) if want_debug else None), "ba_pose_only_mono6")
        nrows = n_it.value - 1 if conv.value else n_it.value
        nrows = max(0, min(nrows, cap))
        return dict(T12=T, mask=m.astype(bool), n_iter=n_it.value,
                    converged=bool(conv.value), success=(rc == 0),
                    rows=[(rows[i].cost, rows[i].cost_change,
                           rows[i].abs_step) for i in range(nrows)],
                    debug=dbg[:min(n_it.value, cap)] if want_debug else None)


    def pose_only_stereo6(self, X3, uvl2, uvr2, intr_l, intr_r, T_lr12, T12,
                          mask_l, mask_r, opt, cap=None, want_debug=False):
        """reference core/pose_only_bundle_adjustment_solver.cpp:172-399."""
        X = np.ascontiguousarray(X3, np.float32).reshape(-1, 3)
        ul = np.ascontiguousarray(uvl2, np.float32).reshape(-1, 2)
        ur = np.ascontiguousarray(uvr2, np.float32).reshape(-1, 2)
        if ul.shape[0] != X.shape[0] or ur.shape[0] != X.shape[0]:
            raise RuntimeError(  # reference :203-214
                "In PoseOnlyBundleAdjustmentSolver::"
                "SolveStereoPoseOnlyBundleAdjustment6Dof(), "
                "world_position_list.size() != current_pixel_list.size()")
        n = X.shape[0]
        il = np.ascontiguousarray(intr_l, np.float32).reshape(4)
        ir = np.ascontiguousarray(intr_r, np.float32).reshape(4)
        Tlr = np.ascontiguousarray(T_lr12, np.float32).reshape(12)
        T = np.ascontiguousarray(T12, np.float32).reshape(12).copy()
        ml = np.ascontiguousarray(mask_l, np.uint8).copy()
        mr = np.ascontiguousarray(mask_r, np.uint8).copy()
        cap = cap or max(1, opt.max_num_iterations)
        rows = (BaPoIter * cap)()
        n_it = C.c_int(0)
        conv = C.c_int(0)
        dbg = np.zeros((cap, 12), np.float32) if want_debug else None
        rc = check(self.lib.ba_pose_only_stereo6(
            self.h, _fp(X), _fp(ul), _fp(ur), n, _fp(il), _fp(ir), _fp(Tlr),
            _fp(T), _up(ml), _up(mr), C.byref(opt), rows, cap, C.byref(n_it),
            C.byref(conv), _fp(dbg) if want_debug else None),
            "ba_pose_only_stereo6")
        nrows = n_it.value - 1 if conv.value else n_it.value
        nrows = max(0, min(nrows, cap))
        return dict(T12=T, mask_l=ml.astype(bool), mask_r=mr.astype(bool),
                    n_iter=n_it.value, converged=bool(conv.value),
                    success=(rc == 0),
                    rows=[(rows[i].cost, rows[i].cost_change,
                           rows[i].abs_step) for i in range(nrows)],
                    debug=dbg[:min(n_it.value, cap)] if want_debug else None)

    def _pose_only_out(self, rc, T, masks, rows, n_it, conv, cap, dbg):
        nrows = n_it.value - 1 if conv.value else n_it.value
        nrows = max(0, min(nrows, cap))
        out = dict(T12=T, n_iter=n_it.value, converged=bool(conv.value),
                   success=(rc == 0),
                   rows=[(rows[i].cost, rows[i].cost_change, rows[i].abs_step)
                         for i in range(nrows)],
                   debug=dbg[:min(n_it.value, cap)] if dbg is not None else None)
        out.update({k: m.astype(bool) for k, m in masks.items()})
        return out

    # -- batched 6-DoF pose-only (ba_pose_only_{mono,stereo}6_batch) --
    @staticmethod
    def _batch_out(T, masks, rows, res, cap, dbg):
        """One dict per problem, in the shape of pose_only_mono6's result."""
        out = []
        for b, r in enumerate(res):
            nrows = max(0, min(r.n_rows, cap))
            d = dict(T12=T[b], n_iter=r.n_iter, converged=bool(r.converged),
                     success=(r.status == 0), status=r.status,
                     rows=[tuple(float(v) for v in rows[b, i]) for i in range(nrows)],
                     debug=dbg[b, :min(r.n_iter, cap)] if dbg is not None else None)
            d.update({k: m[b] for k, m in masks.items()})
            out.append(d)
        return out

    @staticmethod
    def _batch_buffers(what, B, sizes_ok, opt, cap, want_debug):
        """The size check and the output buffers of a numpy batch call: rows
        (B, cap, 3), the ba_po_result array and debug poses (B, cap, 12)."""
        if B >= 1 and not sizes_ok:
            raise ValueError("%s: array sizes do not match offsets" % what)
        cap = cap or max(1, opt.max_num_iterations)
        rows = np.zeros((max(B, 0), cap, 3), np.float32)
        res = (BaPoResult * max(B, 1))()
        dbg = np.zeros((max(B, 0), cap, 12), np.float32) if want_debug else None
        return cap, rows, res, dbg

    def pose_only_mono6_batch(self, offsets, X3, uv2, intr4, T12, mask, opt,
                              cap=None, want_debug=False):
        """B monocular 6-DoF problems in one launch.  offsets (B+1, int32):
        problem b owns rows [offsets[b], offsets[b+1]) of X3 / uv2 / mask;
        intr4 (B, 4) = fx fy cx cy, T12 (B, 12).  Returns one dict per problem
        (T12, mask, n_iter, converged, success, status, rows, debug)."""
        off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        B = off.size - 1
        X = np.ascontiguousarray(X3, np.float32).reshape(-1, 3)
        uv = np.ascontiguousarray(uv2, np.float32).reshape(-1, 2)
        K = np.ascontiguousarray(intr4, np.float32).reshape(-1, 4)
        T = np.ascontiguousarray(T12, np.float32).reshape(-1, 12).copy()
        m = np.ascontiguousarray(mask, np.uint8).reshape(-1).copy()
        cap, rows, res, dbg = self._batch_buffers(
            "pose_only_mono6_batch", B,
            off[-1] == X.shape[0] == uv.shape[0] == m.size and
            K.shape[0] == T.shape[0] == B, opt, cap, want_debug)
        check(self.lib.ba_pose_only_mono6_batch(
            self.h, B, _ip(off), _fp(X), _fp(uv), _fp(K), _fp(T), _up(m),
            C.byref(opt), rows.ctypes.data_as(C.POINTER(BaPoIter)), cap, res,
            _fp(dbg) if want_debug else None), "ba_pose_only_mono6_batch")
        masks = {"mask": [m[off[b]:off[b + 1]].astype(bool) for b in range(B)]}
        return self._batch_out(T, masks, rows, list(res)[:B], cap, dbg)

    def pose_only_stereo6_batch(self, offsets, X3, uvl2, uvr2, intr_l4, intr_r4,
                                T_lr12, T12, mask_l, mask_r, opt, cap=None,
                                want_debug=False):
        """B stereo 6-DoF problems in one launch; as pose_only_mono6_batch plus
        uvr2 (a negative coordinate: no right match), intr_r4 (B, 4), T_lr12
        (B, 12) and the right masks."""
        off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        B = off.size - 1
        X = np.ascontiguousarray(X3, np.float32).reshape(-1, 3)
        ul = np.ascontiguousarray(uvl2, np.float32).reshape(-1, 2)
        ur = np.ascontiguousarray(uvr2, np.float32).reshape(-1, 2)
        Kl = np.ascontiguousarray(intr_l4, np.float32).reshape(-1, 4)
        Kr = np.ascontiguousarray(intr_r4, np.float32).reshape(-1, 4)
        Tlr = np.ascontiguousarray(T_lr12, np.float32).reshape(-1, 12)
        T = np.ascontiguousarray(T12, np.float32).reshape(-1, 12).copy()
        ml = np.ascontiguousarray(mask_l, np.uint8).reshape(-1).copy()
        mr = np.ascontiguousarray(mask_r, np.uint8).reshape(-1).copy()
        cap, rows, res, dbg = self._batch_buffers(
            "pose_only_stereo6_batch", B,
            off[-1] == X.shape[0] == ul.shape[0] == ur.shape[0] == ml.size == mr.size and
            Kl.shape[0] == Kr.shape[0] == Tlr.shape[0] == T.shape[0] == B, opt, cap,
            want_debug)
        check(self.lib.ba_pose_only_stereo6_batch(
            self.h, B, _ip(off), _fp(X), _fp(ul), _fp(ur), _fp(Kl), _fp(Kr),
            _fp(Tlr), _fp(T), _up(ml), _up(mr), C.byref(opt),
            rows.ctypes.data_as(C.POINTER(BaPoIter)), cap, res,
            _fp(dbg) if want_debug else None), "ba_pose_only_stereo6_batch")
        masks = {"mask_l": [ml[off[b]:off[b + 1]].astype(bool) for b in range(B)],
                 "mask_r": [mr[off[b]:off[b + 1]].astype(bool) for b in range(B)]}
        return self._batch_out(T, masks, rows, list(res)[:B], cap, dbg)

    def _tensor_args(self, what, specs):
        """Check (name, tensor, dtype) triples: on this handle's GPU, the dtype,
        contiguous.  Raises ValueError."""
        import torch
        dev = torch.device("cuda", self.device)
        for name, t, dtype in specs:
            if not isinstance(t, torch.Tensor):
                raise ValueError("%s: %s must be a torch.Tensor" % (what, name))
            if t.dtype != dtype:
                raise ValueError("%s: %s must be %s, got %s" % (what, name, dtype, t.dtype))
            if t.device != dev:
                raise ValueError("%s: %s must be on %s, got %s" % (what, name, dev, t.device))
            if not t.is_contiguous():
                raise ValueError("%s: %s must be contiguous" % (what, name))

    @staticmethod
    def right_camera_records(intr_r4, T_lr12):
        """(B, 16) right-camera records of ba_pose_only_stereo6_batch_device from
        intr_r4 (B, 4) and T_lr12 (B, 12) torch tensors, on their device and
        stream: the fp32 operations of ba_right_camera_record, one rounding each
        (so the same bits)."""
        import torch
        B = T_lr12.shape[0]
        R = T_lr12[:, :9].reshape(B, 3, 3).transpose(1, 2)   # left_to_right^-1
        t = T_lr12[:, 9:]
        tr = -((R[:, :, 0] * t[:, 0:1] + R[:, :, 1] * t[:, 1:2]) + R[:, :, 2] * t[:, 2:3])
        return torch.cat([intr_r4, R.reshape(B, 9), tr], 1).contiguous()

    def _batch_tensors(self, stereo, offsets, X3, uvl2, uvr2, intr_l4, intr_r4,
                       T_lr12, T12, mask_l, mask_r, opt, cap, want_debug, rec=None):
        # rec given: the planar 3-DoF batch (B x 52 records, see planar_records)
        import torch
        planar = rec is not None
        what = "pose_only_%s%d_batch_tensors" % ("stereo" if stereo else "mono",
                                                3 if planar else 6)
        f32, i32, u8 = torch.float32, torch.int32, torch.uint8
        specs = [("offsets", offsets, i32), ("X3", X3, f32), ("uv2", uvl2, f32),
                 ("intr4", intr_l4, f32), ("T12", T12, f32), ("mask", mask_l, u8)]
        if stereo:
            specs += [("uvr2", uvr2, f32), ("mask_r", mask_r, u8)]
            if not planar:
                specs += [("intr_r4", intr_r4, f32), ("T_lr12", T_lr12, f32)]
        if planar:
            specs += [("rec", rec, f32)]
        self._tensor_args(what, specs)
        if planar and tuple(rec.shape) != (offsets.numel() - 1, 52):
            raise ValueError("%s: rec must be (B, 52), got %s" % (what, tuple(rec.shape)))
        B = offsets.numel() - 1
        if B < 1:
            raise ValueError("%s: offsets must hold B + 1 >= 2 values" % what)
        dev = offsets.device
        cap = cap or max(1, opt.max_num_iterations)
        T = T12.clone()
        ml = mask_l.clone()
        res = torch.zeros((B, 4), dtype=i32, device=dev)
        rows = torch.zeros((B, cap, 3), dtype=f32, device=dev)
        dbg = torch.zeros((B, cap, 12), dtype=f32, device=dev) if want_debug else None
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        out = dict(T12=T, res=res, rows=rows, debug=dbg)
        if planar:
            mr = mask_r.clone() if stereo else None
            if stereo:
                check(self.lib.ba_pose_only_stereo3_batch_device(
                    self.h, B, p(offsets), p(X3), p(uvl2), p(uvr2), p(intr_l4), p(rec),
                    p(T), p(ml), p(mr), C.byref(opt), p(rows), cap, p(res), p(dbg),
                    stream), what)
                out.update(mask_l=ml, mask_r=mr)
            else:
                check(self.lib.ba_pose_only_mono3_batch_device(
                    self.h, B, p(offsets), p(X3), p(uvl2), p(intr_l4), p(rec), p(T),
                    p(ml), C.byref(opt), p(rows), cap, p(res), p(dbg), stream), what)
                out.update(mask=ml)
        elif stereo:
            mr = mask_r.clone()
            camr = self.right_camera_records(intr_r4, T_lr12)
            check(self.lib.ba_pose_only_stereo6_batch_device(
                self.h, B, p(offsets), p(X3), p(uvl2), p(uvr2), p(intr_l4), p(camr),
                p(T), p(ml), p(mr), C.byref(opt), p(rows), cap, p(res), p(dbg),
                stream), what)
            out.update(mask_l=ml, mask_r=mr)
        else:
            check(self.lib.ba_pose_only_mono6_batch_device(
                self.h, B, p(offsets), p(X3), p(uvl2), p(intr_l4), p(T), p(ml),
                C.byref(opt), p(rows), cap, p(res), p(dbg), stream), what)
            out.update(mask=ml)
        return out

    def pose_only_mono6_batch_tensors(self, offsets, X3, uv2, intr4, T12, mask,
                                      opt, cap=None, want_debug=False):
        """pose_only_mono6_batch on torch tensors already on this handle's GPU
        (offsets int32, masks uint8, the rest float32, contiguous), enqueued on
        torch.cuda.current_stream() without a host sync.  Returns new tensors:
        T12 (B, 12), mask (N,), res (B, 4 int32: n_iter, converged, n_rows,
        status), rows (B, cap, 3: cost, cost_change, abs_step), debug (B, cap,
        12) or None."""
        return self._batch_tensors(False, offsets, X3, uv2, None, intr4, None,
                                   None, T12, mask, None, opt, cap, want_debug)

    def pose_only_stereo6_batch_tensors(self, offsets, X3, uvl2, uvr2, intr_l4,
                                        intr_r4, T_lr12, T12, mask_l, mask_r,
                                        opt, cap=None, want_debug=False):
        """The stereo counterpart of pose_only_mono6_batch_tensors (masks
        returned as mask_l / mask_r); the right-camera records are built on the
        device (right_camera_records)."""
        return self._batch_tensors(True, offsets, X3, uvl2, uvr2, intr_l4, intr_r4,
                                   T_lr12, T12, mask_l, mask_r, opt, cap, want_debug)

    # -- batched planar 3-DoF (ba_pose_only_{mono,stereo}3_batch) --
    def pose_only_mono3_batch(self, offsets, X3, uv2, intr4, T_bc12, T_wl12, T12,
                              mask, opt, cap=None, want_debug=False):
        """B monocular planar 3-DoF problems in one launch.  offsets (B+1,
        int32): problem b owns rows [offsets[b], offsets[b+1]) of X3 (base-1
        coordinates) / uv2 / mask; intr4 (B, 4) = fx fy cx cy, T_bc12, T_wl12
        and T12 = world_to_current (B, 12).  Returns one dict per problem, as
        pose_only_mono6_batch."""
        off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        B = off.size - 1
        X = np.ascontiguousarray(X3, np.float32).reshape(-1, 3)
        uv = np.ascontiguousarray(uv2, np.float32).reshape(-1, 2)
        K = np.ascontiguousarray(intr4, np.float32).reshape(-1, 4)
        Tbc = np.ascontiguousarray(T_bc12, np.float32).reshape(-1, 12)
        Twl = np.ascontiguousarray(T_wl12, np.float32).reshape(-1, 12)
        T = np.ascontiguousarray(T12, np.float32).reshape(-1, 12).copy()
        m = np.ascontiguousarray(mask, np.uint8).reshape(-1).copy()
        cap, rows, res, dbg = self._batch_buffers(
            "pose_only_mono3_batch", B,
            off[-1] == X.shape[0] == uv.shape[0] == m.size and
            K.shape[0] == Tbc.shape[0] == Twl.shape[0] == T.shape[0] == B, opt, cap,
            want_debug)
        check(self.lib.ba_pose_only_mono3_batch(
            self.h, B, _ip(off), _fp(X), _fp(uv), _fp(K), _fp(Tbc), _fp(Twl), _fp(T),
            _up(m), C.byref(opt), rows.ctypes.data_as(C.POINTER(BaPoIter)), cap, res,
            _fp(dbg) if want_debug else None), "ba_pose_only_mono3_batch")
        masks = {"mask": [m[off[b]:off[b + 1]].astype(bool) for b in range(B)]}
        return self._batch_out(T, masks, rows, list(res)[:B], cap, dbg)

    def pose_only_stereo3_batch(self, offsets, X3, uvl2, uvr2, intr_l4, intr_r4,
                                T_bc12, T_lr12, T_wl12, T12, mask_l, mask_r, opt,
                                cap=None, want_debug=False):
        """B stereo planar 3-DoF problems in one launch; as pose_only_mono3_batch
        plus uvr2 (a negative coordinate: no right match), intr_r4 (B, 4),
        T_lr12 (B, 12) and the right masks."""
        off = np.ascontiguousarray(offsets, np.int32).reshape(-1)
        B = off.size - 1
        X = np.ascontiguousarray(X3, np.float32).reshape(-1, 3)
        ul = np.ascontiguousarray(uvl2, np.float32).reshape(-1, 2)
        ur = np.ascontiguousarray(uvr2, np.float32).reshape(-1, 2)
        Kl = np.ascontiguousarray(intr_l4, np.float32).reshape(-1, 4)
        Kr = np.ascontiguousarray(intr_r4, np.float32).reshape(-1, 4)
        Tbc = np.ascontiguousarray(T_bc12, np.float32).reshape(-1, 12)
        Tlr = np.ascontiguousarray(T_lr12, np.float32).reshape(-1, 12)
        Twl = np.ascontiguousarray(T_wl12, np.float32).reshape(-1, 12)
        T = np.ascontiguousarray(T12, np.float32).reshape(-1, 12).copy()
        ml = np.ascontiguousarray(mask_l, np.uint8).reshape(-1).copy()
        mr = np.ascontiguousarray(mask_r, np.uint8).reshape(-1).copy()
        cap, rows, res, dbg = self._batch_buffers(
            "pose_only_stereo3_batch", B,
            off[-1] == X.shape[0] == ul.shape[0] == ur.shape[0] == ml.size == mr.size and
            Kl.shape[0] == Kr.shape[0] == Tbc.shape[0] == Tlr.shape[0] == Twl.shape[0] ==
            T.shape[0] == B, opt, cap, want_debug)
        check(self.lib.ba_pose_only_stereo3_batch(
            self.h, B, _ip(off), _fp(X), _fp(ul), _fp(ur), _fp(Kl), _fp(Kr), _fp(Tbc),
            _fp(Tlr), _fp(Twl), _fp(T), _up(ml), _up(mr), C.byref(opt),
            rows.ctypes.data_as(C.POINTER(BaPoIter)), cap, res,
            _fp(dbg) if want_debug else None), "ba_pose_only_stereo3_batch")
        masks = {"mask_l": [ml[off[b]:off[b + 1]].astype(bool) for b in range(B)],
                 "mask_r": [mr[off[b]:off[b + 1]].astype(bool) for b in range(B)]}
        return self._batch_out(T, masks, rows, list(res)[:B], cap, dbg)

    @staticmethod
    def planar_records(T_bc12, T_wl12, T12, T_lr12=None, intr_r4=None):
        """(B, 52) float32 planar records of the batched planar tensor path,
        one per problem, from ba_planar_record (the host set-up of the single
        planar calls: the prior's psi comes from the host's atan2, so the
        records are built here, not on the device).  T_lr12 / intr_r4 (B, 12) /
        (B, 4): stereo; None for mono (stereo fields zero)."""
        lib = _lib.load()
        Tbc = np.ascontiguousarray(T_bc12, np.float32).reshape(-1, 12)
        Twl = np.ascontiguousarray(T_wl12, np.float32).reshape(-1, 12)
        T = np.ascontiguousarray(T12, np.float32).reshape(-1, 12)
        B = T.shape[0]
        stereo = T_lr12 is not None
        if stereo != (intr_r4 is not None):
            raise ValueError("planar_records: give both T_lr12 and intr_r4, or neither")
        Tlr = np.ascontiguousarray(T_lr12, np.float32).reshape(-1, 12) if stereo else None
        Kr = np.ascontiguousarray(intr_r4, np.float32).reshape(-1, 4) if stereo else None
        if not (Tbc.shape[0] == Twl.shape[0] == B and
                (not stereo or Tlr.shape[0] == Kr.shape[0] == B)):
            raise ValueError("planar_records: arrays must all hold B rows")
        out = np.zeros((B, 52), np.float32)
        for b in range(B):
            check(lib.ba_planar_record(
                _fp(Tbc[b]), _fp(Twl[b]), _fp(T[b]), _fp(Tlr[b]) if stereo else None,
                _fp(Kr[b]) if stereo else None, _fp(out[b])), "ba_planar_record")
        return out

    def pose_only_mono3_batch_tensors(self, offsets, X3, uv2, intr4, rec, T12, mask,
                                      opt, cap=None, want_debug=False):
        """pose_only_mono3_batch on torch tensors already on this handle's GPU
        (offsets int32, mask uint8, the rest float32, contiguous), enqueued on
        torch.cuda.current_stream() without a host sync.  rec (B, 52) holds the
        planar records (planar_records, moved to the device): the device entry
        point never reads T12, the prior comes from the record.  Returns new
        tensors as pose_only_mono6_batch_tensors; T12 keeps its input rows where
        the single call would not write them."""
        return self._batch_tensors(False, offsets, X3, uv2, None, intr4, None, None, T12,
                                   mask, None, opt, cap, want_debug, rec=rec)

    def pose_only_stereo3_batch_tensors(self, offsets, X3, uvl2, uvr2, intr_l4, rec,
                                        T12, mask_l, mask_r, opt, cap=None,
                                        want_debug=False):
        """The stereo counterpart of pose_only_mono3_batch_tensors (records from
        planar_records with T_lr12 and intr_r4; masks returned as mask_l /
        mask_r)."""
        return self._batch_tensors(True, offsets, X3, uvl2, uvr2, intr_l4, None, None, T12,
                                   mask_l, mask_r, opt, cap, want_debug, rec=rec)

    def pose_only_mono3(self, X3, uv2, fx, fy, cx, cy, T_bc12, T_wl12, T12,
                        mask, opt, cap=None, want_debug=False):
        """Planar 3-DoF, reference core/pose_only_bundle_adjustment_solver.cpp:
        401-615.  X3 in base-1 coordinates; T_bc12 = pose_base_to_camera,
        T_wl12 = pose_world_to_last, T12 = pose_world_to_current (returned
        updated as "T12")."""
        X = np.ascontiguousarray(X3, np.float32).reshape(-1, 3)
        uv = np.ascontiguousarray(uv2, np.float32).reshape(-1, 2)
        if uv.shape[0] != X.shape[0]:
            raise RuntimeError(  # reference :426-432
                "In PoseOnlyBundleAdjustmentSolver::"
                "SolveMonocularPoseOnlyBundleAdjustment3Dof(), "
                "world_position_list.size() != current_pixel_list.size()")
        n = X.shape[0]
        Tbc = np.ascontiguousarray(T_bc12, np.float32).reshape(12)
        Twl = np.ascontiguousarray(T_wl12, np.float32).reshape(12)
        T = np.ascontiguousarray(T12, np.float32).reshape(12).copy()
        m = np.ascontiguousarray(mask, np.uint8).copy()
        cap = cap or max(1, opt.max_num_iterations)
        rows = (BaPoIter * cap)()
        n_it = C.c_int(0)
        conv = C.c_int(0)
        dbg = np.zeros((cap, 12), np.float32) if want_debug else None
        rc = check(self.lib.ba_pose_only_mono3(
            self.h, _fp(X), _fp(uv), n, fx, fy, cx, cy, _fp(Tbc), _fp(Twl),
            _fp(T), _up(m), C.byref(opt), rows, cap, C.byref(n_it),
            C.byref(conv), _fp(dbg) if want_debug else None),
            "ba_pose_only_mono3")
        return self._pose_only_out(rc, T, {"mask": m}, rows, n_it, conv, cap, dbg)

    def pose_only_stereo3(self, X3, uvl2, uvr2, intr_l, intr_r, T_bc12,
                          T_lr12, T_wl12, T12, mask_l, mask_r, opt, cap=None,
                          want_debug=False):
        """Planar 3-DoF stereo, reference core/pose_only_bundle_adjustment_
        solver.cpp:617-900 (a right pixel with a negative coordinate: no right
        edge for that point, :785)."""
        X = np.ascontiguousarray(X3, np.float32).reshape(-1, 3)
        ul = np.ascontiguousarray(uvl2, np.float32).reshape(-1, 2)
        ur = np.ascontiguousarray(uvr2, np.float32).reshape(-1, 2)
        for side, u in (("left", ul), ("right", ur)):
            if u.shape[0] != X.shape[0]:
                raise RuntimeError(  # reference :647-660
                    "In PoseOnlyBundleAdjustmentSolver::"
                    "SolveMonocularPoseOnlyBundleAdjustment3Dof(), "
                    "world_position_list.size() != %s_current_pixel_list.size()"
                    % side)
        n = X.shape[0]
        il = np.ascontiguousarray(intr_l, np.float32).reshape(4)
        ir = np.ascontiguousarray(intr_r, np.float32).reshape(4)
        Tbc = np.ascontiguousarray(T_bc12, np.float32).reshape(12)
        Tlr = np.ascontiguousarray(T_lr12, np.float32).reshape(12)
        Twl = np.ascontiguousarray(T_wl12, np.float32).reshape(12)
        T = np.ascontiguousarray(T12, np.float32).reshape(12).copy()
        ml = np.ascontiguousarray(mask_l, np.uint8).copy()
        mr = np.ascontiguousarray(mask_r, np.uint8).copy()
        cap = cap or max(1, opt.max_num_iterations)
        rows = (BaPoIter * cap)()
        n_it = C.c_int(0)
        conv = C.c_int(0)
        dbg = np.zeros((cap, 12), np.float32) if want_debug else None
        rc = check(self.lib.ba_pose_only_stereo3(
            self.h, _fp(X), _fp(ul), _fp(ur), n, _fp(il), _fp(ir), _fp(Tbc),
            _fp(Tlr), _fp(Twl), _fp(T), _up(ml), _up(mr), C.byref(opt), rows,
            cap, C.byref(n_it), C.byref(conv),
            _fp(dbg) if want_debug else None), "ba_pose_only_stereo3")
        return self._pose_only_out(rc, T, {"mask_l": ml, "mask_r": mr}, rows,
                                   n_it, conv, cap, dbg)


def _i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _point_only_structure(what, n_pt, obs_cam, obs_pose, obs_pt, obs_uv):
    """Observations in any order -> the landmark-major lists of ba_point_only: a stable
    sort by point (a landmark keeps the caller's order of its observations) and the
    offsets.  Returns (obs_off, cam, pose, uv, order)."""
    pt = np.asarray(obs_pt, np.int64).reshape(-1)
    cam = np.asarray(obs_cam, np.int32).reshape(-1)
    pose = np.asarray(obs_pose, np.int32).reshape(-1)
    uv = np.asarray(obs_uv, np.float64).reshape(-1, 2)
    if not (pt.size == cam.size == pose.size == uv.shape[0]):
        raise ValueError("%s: observation arrays differ in length" % what)
    if pt.size and (pt.min() < 0 or pt.max() >= n_pt):
        k = int(np.nonzero((pt < 0) | (pt >= n_pt))[0][0])
        raise ValueError("%s: point index %d out of range at observation %d" % (what, pt[k], k))
    order = np.argsort(pt, kind="stable")
    off = np.zeros(n_pt + 1, np.int64)
    np.cumsum(np.bincount(pt, minlength=n_pt), out=off[1:])
    return (off, np.ascontiguousarray(cam[order]), np.ascontiguousarray(pose[order]),
            np.ascontiguousarray(uv[order]), order)


def point_only_check(n_cam, n_pose, n_pt, obs_off, obs_cam, obs_pose):
    """ba_point_only_check: the host-side validation of ba_point_only's structure (no
    GPU).  Raises BaError naming the landmark / observation."""
    off = np.ascontiguousarray(obs_off, np.int64).reshape(-1)
    cam = np.ascontiguousarray(obs_cam, np.int32).reshape(-1)
    pose = np.ascontiguousarray(obs_pose, np.int32).reshape(-1)
    if off.size != max(n_pt, 0) + 1:
        raise ValueError("point_only_check: obs_off must hold n_pt + 1 entries")
    if off.size and (cam.size < off[-1] or pose.size < off[-1]):
        raise ValueError("point_only_check: fewer observations than obs_off[-1]")
    check(_lib.load().ba_point_only_check(n_cam, n_pose, n_pt, _i64p(off), _ip(cam), _ip(pose)),
          "ba_point_only_check")
    return True


def point_only_team(width=0):
    """ba_point_only_team: lanes per landmark of the point-only kernel (8 or 16; 0 asks)."""
    return check(_lib.load().ba_point_only_team(int(width)), "ba_point_only_team")


def point_only_last_ms():
    """device time of this thread's last point_only launch (hipEvents), milliseconds"""
    ms = C.c_double(0.0)
    check(_lib.load().ba_point_only_last_ms(C.byref(ms)), "ba_point_only_last_ms")
    return ms.value


def point_only(handle, cam_intr, cam_T, pose_T, X3, obs_cam, obs_pose, obs_pt, obs_uv, opt,
               triangulate=None, cap=None):
    """ba_point_only on the device and stream of `handle` (a BaProblem): every pose fixed,
    every landmark solved on its own, all in one launch; scaled units.  Observations come
    in any order and are stable-sorted by point.  triangulate: None, or n_pt flags.
    cap: iteration rows kept per landmark (None: max_num_iterations; 0: none).
    Returns (X (n_pt, 3), results, rows): results a numpy record array with the fields
    of ba_point_result, rows one list of BaIterInfo per landmark (None when cap is 0)."""
    K = np.ascontiguousarray(cam_intr, np.float64).reshape(-1, 4)
    Tc = np.ascontiguousarray(cam_T, np.float64).reshape(-1, 12)
    Tp = np.ascontiguousarray(pose_T, np.float64).reshape(-1, 12)
    X = np.ascontiguousarray(X3, np.float64).reshape(-1, 3).copy()
    if K.shape[0] != Tc.shape[0]:
        raise ValueError("point_only: cam_intr and cam_T differ in length")
    n_pt = X.shape[0]
    off, cam, pose, uv, _ = _point_only_structure("point_only", n_pt, obs_cam, obs_pose,
                                                  obs_pt, obs_uv)
    tri = None
    if triangulate is not None:
        tri = np.ascontiguousarray(triangulate, np.uint8).reshape(-1)
        if tri.size != n_pt:
            raise ValueError("point_only: triangulate must hold one flag per point")
    if cap is None:
        cap = max(0, opt.max_num_iterations)
    rows = (BaIterInfo * (max(n_pt, 1) * cap))() if cap > 0 else None
    res = (BaPointResult * max(n_pt, 1))()
    check(handle.lib.ba_point_only(
        handle.h, K.shape[0], _dp(K), _dp(Tc), Tp.shape[0], _dp(Tp), n_pt, _i64p(off),
        _ip(cam), _ip(pose), _dp(uv), _up(tri) if tri is not None else None, _dp(X),
        C.byref(opt), rows, cap, res), "ba_point_only")
    rec = np.frombuffer(res, dtype=np.dtype(BaPointResult), count=max(n_pt, 1))[:n_pt]
    rec = rec.view(np.recarray)
    out_rows = None
    if rows is not None:
        out_rows = [[rows[i * cap + k] for k in range(min(int(rec.n_rows[i]), cap))]
                    for i in range(n_pt)]
    return X, rec, out_rows


class BaBatch:
    """B independent small full-BA problems solved in ONE launch, one persistent
    workgroup each (ba_batch_* of include/ba_hip.h).  `problems`: a list of dicts in
    the layout of scenes.scaled_problem (scaled units, problem-local indices).  The
    structure is planned once; update_values + solve re-optimise new values.  Limits
    per problem: 16 optimisable poses, 64 poses, 8 cameras (status 2 otherwise)."""

    def __init__(self, problems, device=0):
        self.lib = _lib.load()
        self.b = None
        self._owner = BaProblem(device)   # the handle: device and stream
        self.B = len(problems)
        cat = lambda key, dt, w: np.ascontiguousarray(np.concatenate(
            [np.asarray(p[key], dt).reshape((-1,) + w) for p in problems] or
            [np.zeros((0,) + w, dt)], axis=0))
        off = lambda key, dt: np.concatenate(
            [[0], np.cumsum([len(p[key]) for p in problems])]).astype(dt)
        self.cam_off = off("cam_intr", np.int32)
        self.pose_off = off("pose_fixed", np.int32)
        self.pt_off = off("pt_fixed", np.int32)
        self.obs_off = off("obs_cam", np.int64)
        a = dict(cam_intr=cat("cam_intr", np.float64, (4,)), cam_T=cat("cam_T", np.float64, (12,)),
                 pose_T=cat("pose_T", np.float64, (12,)), pose_fixed=cat("pose_fixed", np.uint8, ()),
                 pt_X=cat("pt_X", np.float64, (3,)), pt_fixed=cat("pt_fixed", np.uint8, ()),
                 obs_cam=cat("obs_cam", np.int32, ()), obs_pose=cat("obs_pose", np.int32, ()),
                 obs_pt=cat("obs_pt", np.int32, ()), obs_uv=cat("obs_uv", np.float64, (2,)))
        self.n_pose, self.n_pt = a["pose_T"].shape[0], a["pt_X"].shape[0]
        self._n_rel = 0   # factors given to set_relative (the length of relative_marg_plan's output)
        self.pose_fixed = a["pose_fixed"]
        b = C.c_void_p()
        check(self.lib.ba_batch_create(
            C.byref(b), self._owner.h, self.B, _ip(self.cam_off), _ip(self.pose_off),
            _ip(self.pt_off), self.obs_off.ctypes.data_as(C.POINTER(C.c_int64)),
            _dp(a["cam_intr"]), _dp(a["cam_T"]), _dp(a["pose_T"]), _up(a["pose_fixed"]),
            _dp(a["pt_X"]), _up(a["pt_fixed"]), _ip(a["obs_cam"]), _ip(a["obs_pose"]),
            _ip(a["obs_pt"]), _dp(a["obs_uv"])), "ba_batch_create")
        self.b = b

    def close(self):
        if self.b:
            self.lib.ba_batch_destroy(self.b)
            self.b = None
        if self._owner is not None:
            self._owner.close()
            self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, opt, cap=None):
        """-> (rows, results): rows[p] = the logged ba_iter_info rows of problem p,
        results[p] = its BaBatchResult."""
        cap = max(1, opt.max_num_iterations) if cap is None else cap
        rows = (BaIterInfo * max(1, self.B * cap))()
        res = (_lib.BaBatchResult * self.B)()
        check(self.lib.ba_batch_solve(self.b, C.byref(opt), rows, cap, res), "ba_batch_solve")
        out = [[rows[p * cap + i] for i in range(min(res[p].n_rows, cap))]
               for p in range(self.B)]
        return out, [res[p] for p in range(self.B)]

    def covariance(self, huber, points=True):
        """-> (cov_pose [n_pose, 6, 6], cov_pt [n_pt, 3, 3] or None, results): the
        covariance blocks of every problem at the values the object holds, one
        launch (ba_batch_covariance; scaled units, concatenated user order, blocks
        of fixed members zero), results[p] = its BaBatchCovResult."""
        cp = np.zeros((self.n_pose, 6, 6))
        cq = np.zeros((self.n_pt, 3, 3)) if points else None
        res = (_lib.BaBatchCovResult * self.B)()
        check(self.lib.ba_batch_covariance(self.b, float(huber), _dp(cp),
                                           _dp(cq) if points else None, res),
              "ba_batch_covariance")
        return cp, cq, [res[p] for p in range(self.B)]

    def _marking(self, marg_pose):
        m = np.ascontiguousarray(np.asarray(marg_pose).reshape(-1) != 0, np.uint8)
        if m.shape[0] != self.n_pose:
            raise ValueError("marg_pose: one byte per pose of the batch (%d)" % self.n_pose)
        return m

    def marg_layout(self, marg_pose):
        """-> (H_off, b_off): element offsets (B + 1 each) of every problem's prior
        in the outputs of ba_batch_marginalize for this marking (host only)."""
        m = self._marking(marg_pose)
        Ho, bo = np.zeros(self.B + 1, np.int64), np.zeros(self.B + 1, np.int64)
        i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
        check(self.lib.ba_batch_marg_layout(self.b, _up(m), i64(Ho), i64(bo)),
              "ba_batch_marg_layout")
        return Ho, bo

    def marginalize(self, marg_pose, huber):
        """-> (H_list, b_list, kept_list, results): the marginalisation prior of every
        problem at the values the object holds, one launch (ba_batch_marginalize;
        scaled units).  marg_pose: one byte per pose of the batch, concatenated user
        order.  H_list[p] (6K, 6K) and b_list[p] (6K,) are views of the two output
        arrays, kept_list[p] the kept poses (problem-local user indices, ascending),
        results[p] its BaBatchMargResult.  self.marg_pt holds the landmark set L of
        the call (one byte per point of the batch)."""
        m = self._marking(marg_pose)
        Ho, bo = self.marg_layout(m)
        H = np.zeros(int(Ho[-1]))
        bv = np.zeros(int(bo[-1]))
        self.marg_pt = np.zeros(self.n_pt, np.uint8)
        res = (_lib.BaBatchMargResult * self.B)()
        check(self.lib.ba_batch_marginalize(
            self.b, float(huber), _up(m), _dp(H) if H.size else None,
            _dp(bv) if bv.size else None, _up(self.marg_pt), res), "ba_batch_marginalize")
        Hl, bl, kl = [], [], []
        for p in range(self.B):
            K6 = int(bo[p + 1] - bo[p])
            Hl.append(H[Ho[p]:Ho[p + 1]].reshape(K6, K6))
            bl.append(bv[bo[p]:bo[p + 1]])
            sl = slice(self.pose_off[p], self.pose_off[p + 1])
            kl.append(np.flatnonzero((self.pose_fixed[sl] == 0) & (m[sl] == 0)).astype(np.int32))
        return Hl, bl, kl, [res[p] for p in range(self.B)]

    def set_prior(self, priors):
        """One pose prior per problem (ba_batch_set_prior; scaled units).  priors: a list
        with one entry per problem, each None or a dict with the keys
          poses  problem-local user indices of K optimisable poses, strictly ascending,
          H      (6K, 6K), only the lower triangle is read,   b  (6K,),
          T_lin  (K, 12) the poses at which H and b were formed,   c  >= 0 (default 0).
        The prior stays with the object until clear_prior or the next set_prior."""
        if len(priors) != self.B:
            raise ValueError("set_prior: one entry (or None) per problem (%d)" % self.B)
        off = np.zeros(self.B + 1, np.int32)
        pose, Tl, Hs, bs = [], [], [], []
        c = np.zeros(self.B)
        for p, pr in enumerate(priors):
            K = 0
            if pr is not None:
                idx = np.asarray(pr["poses"], np.int32).reshape(-1)
                K = idx.shape[0]
                H = np.asarray(pr["H"], np.float64)
                b = np.asarray(pr["b"], np.float64).reshape(-1)
                T = np.asarray(pr["T_lin"], np.float64).reshape(-1, 12)
                if H.shape != (6 * K, 6 * K) or b.shape != (6 * K,) or T.shape != (K, 12):
                    raise ValueError("set_prior: problem %d needs H (6K, 6K), b (6K,), "
                                     "T_lin (K, 12) for its K = %d poses" % (p, K))
                pose.append(idx)
                Tl.append(T.reshape(-1))
                Hs.append(H.reshape(-1))
                bs.append(b)
                c[p] = float(pr.get("c", 0.0))
            off[p + 1] = off[p] + K
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs or [np.zeros(0, dt)]), dt)
        pose, Tl, Hs, bs = cat(pose, np.int32), cat(Tl, np.float64), cat(Hs, np.float64), cat(bs, np.float64)
        check(self.lib.ba_batch_set_prior(self.b, _ip(off), _ip(pose), _dp(Tl), _dp(Hs), _dp(bs), _dp(c)),
              "ba_batch_set_prior")

    def clear_prior(self):
        check(self.lib.ba_batch_set_prior(self.b, None, None, None, None, None, None),
              "ba_batch_set_prior")

    def prior_info(self):
        o = (C.c_int64 * 4)()
        check(self.lib.ba_batch_prior_info(self.b, o), "ba_batch_prior_info")
        return dict(n_prior=int(o[0]), total_K=int(o[1]), device_bytes=int(o[2]))

    def set_relative(self, rels):
        """Relative-pose factors per problem (ba_batch_set_relative; scaled units).  rels:
        a list with one entry per problem, each None or a dict with the keys
          j, k    (F,) problem-local user indices of two distinct poses, at least one of
                  them optimisable (a fixed pose receives nothing),
          Z       (F, 12) the measurement of T_j T_k^-1,
          Omega   (F, 6, 6) information matrices, only the lower triangle is read.
        Residual se3_log(T_j T_k^-1 Z^-1), first-order Jacobians I and -Ad(T_j T_k^-1); no
        robust weight.  Several factors may name one pair.  The factors stay with the
        object until clear_relative or the next set_relative."""
        if len(rels) != self.B:
            raise ValueError("set_relative: one entry (or None) per problem (%d)" % self.B)
        off = np.zeros(self.B + 1, np.int32)
        js, ks, Zs, Os = [], [], [], []
        for p, rl in enumerate(rels):
            F = 0
            if rl is not None:
                refuse_robust("set_relative: problem %d" % p, rl)
                j = np.asarray(rl["j"], np.int32).reshape(-1)
                k = np.asarray(rl["k"], np.int32).reshape(-1)
                F = j.shape[0]
                Z = np.asarray(rl["Z"], np.float64).reshape(-1, 12)
                Om = np.asarray(rl["Omega"], np.float64).reshape(-1, 36)
                if k.shape != (F,) or Z.shape != (F, 12) or Om.shape != (F, 36):
                    raise ValueError("set_relative: problem %d needs j (F,), k (F,), Z (F, 12), "
                                     "Omega (F, 6, 6) for its F = %d factors" % (p, F))
                js.append(j)
                ks.append(k)
                Zs.append(Z.reshape(-1))
                Os.append(Om.reshape(-1))
            off[p + 1] = off[p] + F
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs or [np.zeros(0, dt)]), dt)
        js, ks, Zs, Os = cat(js, np.int32), cat(ks, np.int32), cat(Zs, np.float64), cat(Os, np.float64)
        # the validation first, on the host: a refusal leaves the factors set before in effect
        check(self.lib.ba_batch_relative_check(self.B, _ip(self.pose_off), _up(self.pose_fixed), _ip(off), _ip(js),
                                               _ip(ks), _dp(Zs), _dp(Os)), "ba_batch_relative_check")
        rc = self.lib.ba_batch_set_relative(self.b, _ip(off), _ip(js), _ip(ks), _dp(Zs), _dp(Os))
        self._n_rel = int(off[-1]) if rc == 0 else 0   # a call that fails now leaves the batch without factors
        check(rc, "ba_batch_set_relative")

    def clear_relative(self):
        check(self.lib.ba_batch_set_relative(self.b, None, None, None, None, None),
              "ba_batch_set_relative")
        self._n_rel = 0

    def relative_info(self):
        o = (C.c_int64 * 4)()
        check(self.lib.ba_batch_relative_info(self.b, o), "ba_batch_relative_info")
        return dict(n_problems=int(o[0]), n_factors=int(o[1]), device_bytes=int(o[2]))

    def relative_marg_plan(self, marg_pose):
        """-> one byte per factor given to set_relative, input order: 1 where the factor
        joins marginalize under this marking (one of its poses is marked) and leaves with
        the marked poses, 0 where the caller carries it into the next window."""
        m = self._marking(marg_pose)
        out = np.zeros(self._n_rel, np.uint8)
        check(self.lib.ba_batch_relative_marg_plan(self.b, _up(m), _up(out)),
              "ba_batch_relative_marg_plan")
        return out

    # ---- observation report, mask and cull (ba_batch_obs_report, ba_batch_set_obs_mask,
    # ba_batch_cull, ba_batch_solve_culled); observations in user order throughout
    @property
    def n_obs(self):
        return int(self.obs_off[-1])

    def obs_of(self, p, a):
        """the entries of problem p in a per-observation array of the batch"""
        return a[int(self.obs_off[p]):int(self.obs_off[p + 1])]

    def obs_report(self, huber):
        """-> per problem a dict of views {r2 (n, 2), e2, w, depth}: every observation at the
        values the object holds, user order, scaled units; off observations included."""
        n = self.n_obs
        r2, e2, w, dp = np.zeros((n, 2)), np.zeros(n), np.zeros(n), np.zeros(n)
        check(self.lib.ba_batch_obs_report(self.b, float(huber), _dp(r2), _dp(e2), _dp(w), _dp(dp)),
              "ba_batch_obs_report")
        return [dict(r2=self.obs_of(p, r2), e2=self.obs_of(p, e2), w=self.obs_of(p, w),
                     depth=self.obs_of(p, dp)) for p in range(self.B)]

    def _obs_flags(self, what, masks):
        """one flag per observation of the batch from a flat array or one array per problem"""
        if isinstance(masks, (list, tuple)) and len(masks) == self.B and not np.isscalar(masks[0]):
            for p, m in enumerate(masks):
                want = int(self.obs_off[p + 1] - self.obs_off[p])
                if np.asarray(m).reshape(-1).shape[0] != want:
                    raise ValueError("%s: problem %d has %d observations, its mask %d flags"
                                     % (what, p, want, np.asarray(m).reshape(-1).shape[0]))
            masks = np.concatenate([np.asarray(m).reshape(-1) != 0 for m in masks] or [np.zeros(0, bool)])
        m = np.ascontiguousarray(np.asarray(masks).reshape(-1) != 0, np.uint8)
        if m.shape[0] != self.n_obs:
            raise ValueError("%s: one flag per observation of the batch (%d), got %d"
                             % (what, self.n_obs, m.shape[0]))
        return m

    def set_obs_mask(self, masks):
        """masks: None (clears the mask), one flag per observation of the batch, or a list
        with one flag array per problem; non-zero = on."""
        if masks is None:
            check(self.lib.ba_batch_set_obs_mask(self.b, None), "ba_batch_set_obs_mask")
            return
        m = self._obs_flags("set_obs_mask", masks)
        check(self.lib.ba_batch_set_obs_mask(self.b, _up(m)), "ba_batch_set_obs_mask")

    def get_obs_mask(self):
        """-> per problem a bool view of the mask in effect (all True without one)"""
        m = np.ones(self.n_obs, np.uint8)
        check(self.lib.ba_batch_get_obs_mask(self.b, _up(m)), "ba_batch_get_obs_mask")
        m = m != 0
        return [self.obs_of(p, m) for p in range(self.B)]

    @staticmethod
    def cull_options(e2_max, cull_behind=True):
        """-> BaCullOptions, refused as ba_batch_cull_check refuses (host only)"""
        c = _lib.BaCullOptions(float(e2_max), 1 if cull_behind else 0)
        check(_lib.load().ba_batch_cull_check(C.byref(c)), "ba_batch_cull_check")
        return c

    def cull(self, e2_max, cull_behind=True):
        """Switches off every on observation with !(e2 <= e2_max), or behind its camera, at
        the held values; -> one BaBatchCullResult per problem."""
        c = self.cull_options(e2_max, cull_behind)
        cres = (_lib.BaBatchCullResult * self.B)()
        check(self.lib.ba_batch_cull(self.b, C.byref(c), cres), "ba_batch_cull")
        return [cres[p] for p in range(self.B)]

    @staticmethod
    def solve_culled_cap(first, second, cap=None):
        """the row capacity of solve_culled, refused as ba_batch_solve_culled refuses it"""
        if first is None or second is None:
            raise ValueError("solve_culled: null options")
        n1, n2 = int(first.max_num_iterations), int(second.max_num_iterations)
        if n1 <= 0 or n2 <= 0:
            raise ValueError("solve_culled: both stages need max_num_iterations >= 1")
        cap = n1 + n2 if cap is None else int(cap)
        if cap < n1 + n2:
            raise ValueError("solve_culled: cap = %d is less than the iterations of both stages "
                             "(%d + %d)" % (cap, n1, n2))
        return cap

    def solve_culled(self, first, second, e2_max, cull_behind=True, cap=None):
        """solve(first); cull; solve(second) in one go, no host synchronisation in between.
        -> (rows_first, results_first, rows, results, cull_results), each per problem."""
        cap = self.solve_culled_cap(first, second, cap)
        c = self.cull_options(e2_max, cull_behind)
        rows = (BaIterInfo * max(1, self.B * cap))()
        r1 = (_lib.BaBatchResult * self.B)()
        r2 = (_lib.BaBatchResult * self.B)()
        cres = (_lib.BaBatchCullResult * self.B)()
        check(self.lib.ba_batch_solve_culled(self.b, C.byref(first), C.byref(second), C.byref(c), rows,
                                             cap, r1, r2, cres), "ba_batch_solve_culled")
        off = int(first.max_num_iterations)
        rows1 = [[rows[p * cap + i] for i in range(min(r1[p].n_rows, off))] for p in range(self.B)]
        rows2 = [[rows[p * cap + off + i] for i in range(min(r2[p].n_rows, cap - off))]
                 for p in range(self.B)]
        B = range(self.B)
        return rows1, [r1[p] for p in B], rows2, [r2[p] for p in B], [cres[p] for p in B]

    def cov_poses_of(self, p, cov_pose):
        return cov_pose[self.pose_off[p]:self.pose_off[p + 1]]

    def cov_points_of(self, p, cov_pt):
        return cov_pt[self.pt_off[p]:self.pt_off[p + 1]]

    def update_values(self, T_jw12=None, X3=None):
        T = None if T_jw12 is None else np.ascontiguousarray(T_jw12, np.float64).reshape(-1, 12)
        X = None if X3 is None else np.ascontiguousarray(X3, np.float64).reshape(-1, 3)
        if T is not None and T.shape[0] != self.n_pose or X is not None and X.shape[0] != self.n_pt:
            raise ValueError("update_values: the structure is fixed (same number of poses / points)")
        check(self.lib.ba_batch_update_values(self.b, None if T is None else _dp(T),
                                              None if X is None else _dp(X)),
              "ba_batch_update_values")

    def get_poses(self):
        """every pose of the batch, concatenated user order [n_pose, 12]"""
        T = np.zeros((self.n_pose, 12))
        check(self.lib.ba_batch_get_poses(self.b, _dp(T)), "ba_batch_get_poses")
        return T

    def get_points(self):
        X = np.zeros((self.n_pt, 3))
        check(self.lib.ba_batch_get_points(self.b, _dp(X)), "ba_batch_get_points")
        return X

    def poses_of(self, p, T=None):
        T = self.get_poses() if T is None else T
        return T[self.pose_off[p]:self.pose_off[p + 1]]

    def points_of(self, p, X=None):
        X = self.get_points() if X is None else X
        return X[self.pt_off[p]:self.pt_off[p + 1]]

    def info(self):
        o = (C.c_int64 * 8)()
        check(self.lib.ba_batch_info(self.b, o), "ba_batch_info")
        keys = ("scratch_bytes_max", "lds_bytes", "max_opt_poses", "max_poses", "max_cameras",
                "image_columns", "device_bytes", "B")
        out = dict(zip(keys, [int(v) for v in o]))
        per = (C.c_int64 * self.B)()
        check(self.lib.ba_batch_scratch_bytes(self.b, per), "ba_batch_scratch_bytes")
        out["scratch_bytes"] = [int(v) for v in per]    # per problem
        return out


ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_GEMAN_MCCLURE = 0, 1, 2, 3


def _robust_arrays(kind, scale, n_rel=None):
    """kind (F,) int32 or None, scale (F,) float64 (None: zeros, for kinds that are all 0)"""
    if kind is None:
        return None, None
    kd = np.ascontiguousarray(kind, np.int32).reshape(-1)
    sc = np.zeros(len(kd)) if scale is None else np.ascontiguousarray(scale, np.float64).reshape(-1)
    if len(sc) != len(kd) or (n_rel is not None and len(kd) != n_rel):
        raise ValueError("robust kernels: one kind and one scale per factor")
    return kd, sc


def pgraph_robust_check(kind, scale):
    """Host-only validation of BaPoseGraph.set_robust's inputs (ba_pgraph_robust_check); raises BaError."""
    kd, sc = _robust_arrays(kind, scale)
    n = 0 if kd is None else len(kd)
    check(_lib.load().ba_pgraph_robust_check(n, None if kd is None else _ip(kd), None if sc is None else _dp(sc)),
          "ba_pgraph_robust_check")


def refuse_robust(what, rels):
    """The BA paths (handle, batch) take no robust kernel: a factor dict that carries one is
    refused, not silently solved with full weight."""
    kd = None if rels is None else rels.get("robust_kind")
    if kd is not None and np.any(np.asarray(kd) != 0):
        f = int(np.flatnonzero(np.asarray(kd).reshape(-1) != 0)[0])
        raise _lib.BaError("%s: factor %d carries a robust kernel; robust factors are pose-graph only "
                           "(SolvePoseGraph, BaPoseGraph.set_robust)" % (what, f))


def _graph_arrays(pose, pose_fixed, rels, W):
    """The arrays of a graph of tangent width W as the library reads them: poses (n, W + 6), pose_fixed
    (n,) uint8 or None, j (F,), k (F,), Z (F, W + 6), Omega (F, W W)"""
    P = np.ascontiguousarray(pose, np.float64).reshape(-1, W + 6)
    fx = None if pose_fixed is None else np.ascontiguousarray(pose_fixed, np.uint8).reshape(-1)
    j = np.ascontiguousarray(rels["j"], np.int32).reshape(-1)
    k = np.ascontiguousarray(rels["k"], np.int32).reshape(-1)
    Z = np.ascontiguousarray(rels["Z"], np.float64).reshape(-1, W + 6)
    Om = np.ascontiguousarray(rels["Omega"], np.float64).reshape(-1, W * W)
    return P, fx, j, k, Z, Om


def _graph_check(abi, W, pose, pose_fixed, rels):
    P, fx, j, k, Z, Om = _graph_arrays(pose, pose_fixed, rels, W)
    check(getattr(_lib.load(), abi + "_check")(P.shape[0], _dp(P) if P.size else None, None if fx is None else _up(fx),
                                                len(j), _ip(j), _ip(k), _dp(Z), _dp(Om)), abi + "_check")


def pgraph_check(pose_T, pose_fixed, rels):
    """Host-only validation of BaPoseGraph's inputs (ba_pgraph_check); raises BaError."""
    _graph_check("ba_pgraph", 6, pose_T, pose_fixed, rels)


def _pair_arrays(pairs):
    """pairs: None, or (j, k) index arrays, or an (n, 2) array -> (j, k) int32"""
    if pairs is None:
        return np.zeros(0, np.int32), np.zeros(0, np.int32)
    if isinstance(pairs, tuple) and len(pairs) == 2 and np.ndim(pairs[0]) == 1:
        j, k = pairs
    else:
        jk = np.asarray(pairs, np.int64).reshape(-1, 2)
        j, k = jk[:, 0], jk[:, 1]
    j = np.ascontiguousarray(j, np.int32).reshape(-1)
    k = np.ascontiguousarray(k, np.int32).reshape(-1)
    if len(j) != len(k):
        raise ValueError("pairs: one j and one k per pair")
    return j, k


def _candidate_arrays(j, k, Z, Omega, W):
    j, k = _pair_arrays((np.atleast_1d(j), np.atleast_1d(k)))
    Z = np.ascontiguousarray(Z, np.float64).reshape(-1, W + 6)
    Om = np.ascontiguousarray(Omega, np.float64).reshape(-1, W * W)
    if Z.shape[0] != len(j) or Om.shape[0] != len(j):
        raise ValueError("candidates: needs j (n,), k (n,), Z (n, %d), Omega (n, %d, %d)" % (W + 6, W, W))
    return j, k, Z, Om


def _graph_cov_check(abi, W, n_pose, pose_fixed, pose_sel, pairs, candidates):
    fx = None if pose_fixed is None else np.ascontiguousarray(pose_fixed, np.uint8).reshape(-1)
    ps = np.zeros(0, np.int32) if pose_sel is None else np.ascontiguousarray(pose_sel, np.int32).reshape(-1)
    pj, pk = _pair_arrays(pairs)
    c = candidates
    cj, ck, Z, Om = _candidate_arrays(c["j"], c["k"], c["Z"], c["Omega"], W) if c is not None else \
        _candidate_arrays([], [], np.zeros((0, W + 6)), np.zeros((0, W * W)), W)
    out = np.zeros(1)   # the outputs only have to be there
    check(getattr(_lib.load(), abi + "_cov_check")(int(n_pose), None if fx is None else _up(fx), len(ps), _ip(ps),
                                                    _dp(out), len(pj), _ip(pj), _ip(pk), _dp(out), len(cj), _ip(cj),
                                                    _ip(ck), _dp(Z) if Z.size else None, _dp(Om) if Om.size else None,
                                                    _dp(out)), abi + "_cov_check")


def pgraph_cov_check(n_pose, pose_fixed, pose_sel=None, pairs=None, candidates=None):
    """Host-only validation of BaPoseGraph.covariance / gate (ba_pgraph_cov_check); raises BaError.
    pose_sel: user indices; pairs: (j, k) arrays or (n, 2); candidates: dict(j, k, Z, Omega)."""
    _graph_cov_check("ba_pgraph", 6, n_pose, pose_fixed, pose_sel, pairs, candidates)


class _BaGraph:
    """What BaPoseGraph and BaSim3Graph share: every method but the ones that carry a kind's own
    argument names.  A kind is its ABI prefix, its tangent width W (W + 6 doubles per pose and per
    measurement Z, W x W per Omega and per covariance block) and the keys of its info() words; the
    library behind it is one driver too (csrc/ba_graph.hip)."""

    _abi, _W, _pose_arg = None, 0, None
    _info_keys = ("N", "factors", "blocks", "nb", "tiles", "levels", "image_bytes", "bad_pivots")

    def _call(self, entry, *args):
        name = "%s_%s" % (self._abi, entry)
        check(getattr(self.lib, name)(*args), name)

    def __init__(self, pose, pose_fixed, rels, device=0, owner=None):
        self.lib = _lib.load()
        self.g = None
        self._own = owner is None
        self._owner = None
        W = self._W
        P, fx, j, k, Z, Om = _graph_arrays(pose, pose_fixed, rels, W)
        if not (len(k) == len(j) and Z.shape[0] == len(j) and Om.shape[0] == len(j)) or \
                (fx is not None and len(fx) != P.shape[0]):
            raise ValueError("%s: needs %s (n, %d), pose_fixed (n,), j (F,), k (F,), Z (F, %d), Omega (F, %d, %d)"
                             % (type(self).__name__, self._pose_arg, W + 6, W + 6, W, W))
        _graph_check(self._abi, W, P, fx, dict(j=j, k=k, Z=Z, Omega=Om))   # refusals need no device
        self.n_pose, self.n_rel = P.shape[0], len(j)
        self._fixed = np.zeros(self.n_pose, np.uint8) if fx is None else fx.copy()
        self._owner = BaProblem(device) if owner is None else owner
        g = C.c_void_p()
        self._call("create", C.byref(g), self._owner.h, self.n_pose, _dp(P), None if fx is None else _up(fx),
                   self.n_rel, _ip(j), _ip(k), _dp(Z), _dp(Om))
        self.g = g
        if rels.get("robust_kind") is not None:   # a factor dict that carries kernels
            self.set_robust(rels["robust_kind"], rels.get("robust_scale"))

    def set_robust(self, kind, scale=None):
        """Robust kernels of the factors (ba_pgraph_set_robust; ba_sim3_set_robust,
        §6p): kind (F,) of ROBUST_NONE / HUBER / CAUCHY / GEMAN_MCCLURE, scale (F,) the Mahalanobis
        distance c > 0 of each factor whose kind is not 0.  kind None clears every kernel.  No
        re-planning: call it between solves as often as needed."""
        kd, sc = _robust_arrays(kind, scale, self.n_rel)
        self._call("set_robust", self.g, None if kd is None else _ip(kd), None if sc is None else _dp(sc))

    def _factor_sw(self, entry):
        s, w = np.zeros(self.n_rel), np.zeros(self.n_rel)
        self._call(entry, self.g, _dp(s), _dp(w))
        return s, w

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.g:
            getattr(self.lib, self._abi + "_destroy")(self.g)
            self.g = None
        if self._owner is not None and self._own:
            self._owner.close()
        self._owner = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _update_values(self, pose, Z, Omega):
        W = self._W
        P = None if pose is None else np.ascontiguousarray(pose, np.float64).reshape(-1, W + 6)
        Zs = None if Z is None else np.ascontiguousarray(Z, np.float64).reshape(-1, W + 6)
        Om = None if Omega is None else np.ascontiguousarray(Omega, np.float64).reshape(-1, W * W)
        if (P is not None and P.shape[0] != self.n_pose) or (Zs is not None and Zs.shape[0] != self.n_rel) or \
                (Om is not None and Om.shape[0] != self.n_rel):
            raise ValueError("update_values: the structure is fixed (same number of poses / factors)")
        self._call("update_values", self.g, None if P is None else _dp(P), None if Zs is None else _dp(Zs),
                   None if Om is None else _dp(Om))

    def solve(self, opt, cap=None, rows=None):
        """-> (rows, converged): the logged ba_iter_info rows.  rows: a BaIterInfo array to
        write into (then all `cap` entries are returned), or None."""
        cap = max(1, opt.max_num_iterations) if cap is None else cap
        given = rows is not None
        rows = (BaIterInfo * max(1, cap))() if rows is None else rows
        n_iter, conv = C.c_int(0), C.c_int(0)
        self._call("solve", self.g, C.byref(opt), rows, cap, C.byref(n_iter), C.byref(conv))
        self.n_iter = n_iter.value
        n = cap if given else min(n_iter.value, cap)
        return [rows[i] for i in range(n)], bool(conv.value)

    def poses(self):
        P = np.zeros((self.n_pose, self._W + 6))
        self._call("get_poses", self.g, _dp(P))
        return P

    def cost(self):
        v = C.c_double(0.0)
        self._call("cost", self.g, C.byref(v))
        return v.value

    def system(self):
        """-> (H (W N, W N), g (W N,)): the undamped system at the poses the object holds (W = 6 on
        BaPoseGraph, 7 on BaSim3Graph)"""
        n = self._W * self.info()["N"]
        H, g = np.zeros((n, n)), np.zeros(n)
        self._call("get_system", self.g, _dp(H), _dp(g))
        return H, g

    def info(self):
        out = (C.c_int64 * len(self._info_keys))()
        self._call("info", self.g, out)
        return {key: int(out[i]) for i, key in enumerate(self._info_keys)}

    def last_ms(self):
        v = C.c_double(0.0)
        self._call("last_ms", self.g, C.byref(v))
        return v.value

    def covariance(self, pose_sel=None, pairs=None):
        """-> (cov_pose (n, W, W), cov_cross (p, W, W), cov_rel (p, W, W)): blocks of the inverse of
        system()'s H at the poses the object holds (ba_pgraph_covariance, DESIGN.md §6m, W = 6;
        ba_sim3_covariance, §6p, W = 7 and tangent [v; omega; sigma]): Sigma_jj per selected pose,
        Sigma_jk and the covariance Sigma_E of T_j T_k^-1 (S_j S_k^-1) per pair.  pose_sel: user
        indices of optimisable poses (None: all of them); pairs: (j, k) arrays or (p, 2).  Scaled
        units.  self.dropped_pivots: non-positive pivots of the factorisation."""
        W = self._W
        ps = np.flatnonzero(self._fixed == 0).astype(np.int32) if pose_sel is None else \
            np.ascontiguousarray(pose_sel, np.int32).reshape(-1)
        pj, pk = _pair_arrays(pairs)
        cp, cc, cr = np.zeros((len(ps), W, W)), np.zeros((len(pj), W, W)), np.zeros((len(pj), W, W))
        dropped = C.c_int64(0)
        self._call("covariance", self.g, len(ps), _ip(ps) if len(ps) else None, _dp(cp) if len(ps) else None,
                   len(pj), _ip(pj) if len(pj) else None, _ip(pk) if len(pj) else None,
                   _dp(cc) if len(pj) else None, _dp(cr) if len(pj) else None, C.byref(dropped))
        self.dropped_pivots = dropped.value
        return cp, cc, cr

    def gate(self, j, k, Z, Omega):
        """-> (d2 (n,), r (n, W), P (n, W, W)) of loop-closure candidates shaped like factors
        (ba_pgraph_gate: r = se3_log(T_j T_k^-1 Z^-1); ba_sim3_gate: r = sim3_log(S_j S_k^-1 Z^-1)):
        P = Sigma_E + Omega^-1, d2 = r^T P^-1 r, to be compared with a chi-square quantile of W
        degrees of freedom (at 0.999: 22.46 for 6, 24.32 for 7)."""
        W = self._W
        cj, ck, Zs, Om = _candidate_arrays(j, k, Z, Omega, W)
        n = len(cj)
        d2, r, P = np.zeros(n), np.zeros((n, W)), np.zeros((n, W, W))
        dropped = C.c_int64(0)
        self._call("gate", self.g, n, _ip(cj) if n else None, _ip(ck) if n else None, _dp(Zs) if n else None,
                   _dp(Om) if n else None, _dp(d2) if n else None, _dp(r) if n else None, _dp(P) if n else None,
                   C.byref(dropped))
        self.dropped_pivots = dropped.value
        return d2, r, P

    def cov_info(self):
        """Column batches of covariance / gate on this graph (BA_COV_BATCH of the borrowed handle overrides)"""
        v = (C.c_int64 * 4)()
        self._call("cov_info", self.g, v)
        return dict(batch_cols=int(v[0]), cols_per_wave=int(v[1]), batches=int(v[2]), workspace_bytes=int(v[3]))


class BaPoseGraph(_BaGraph):
    """Pose-graph optimisation (ba_pgraph_* of include/ba_hip.h): chi-square
    Levenberg-Marquardt over relative-pose factors alone.  pose_T (n, 12) T_jw in scaled
    units, pose_fixed (n,) or None, rels the dict of BaProblem.set_relative.  The structure
    (lists, tile schedule, dense image) is planned once; update_values + solve re-optimise
    new values.  owner: a BaProblem whose handle (device, stream, BA_DENSE_* knobs) is
    borrowed, or None for a handle of its own."""

    _abi, _W, _pose_arg = "ba_pgraph", 6, "pose_T"

    def __init__(self, pose_T, pose_fixed, rels, device=0, owner=None):
        super().__init__(pose_T, pose_fixed, rels, device, owner)

    def update_values(self, pose_T=None, Z=None, Omega=None):
        """New values for the same structure (ba_pgraph_update_values); None keeps."""
        self._update_values(pose_T, Z, Omega)

    def factor_report(self):
        """-> (s (F,), w (F,)): s_f = r_f^T Omega_f r_f and the robust weight w_f of every
        factor at the poses the object holds (ba_pgraph_factor_report)"""
        return self._factor_sw("factor_report")


def sim3_check(pose_S, pose_fixed, rels):
    """Host-only validation of BaSim3Graph's inputs (ba_sim3_check); raises BaError."""
    _graph_check("ba_sim3", 7, pose_S, pose_fixed, rels)


def sim3_robust_check(kind, scale):
    """Host-only validation of BaSim3Graph.set_robust's inputs (ba_sim3_robust_check); raises BaError."""
    kd, sc = _robust_arrays(kind, scale)
    n = 0 if kd is None else len(kd)
    check(_lib.load().ba_sim3_robust_check(n, None if kd is None else _ip(kd), None if sc is None else _dp(sc)),
          "ba_sim3_robust_check")


def sim3_cov_check(n_pose, pose_fixed, pose_sel=None, pairs=None, candidates=None):
    """Host-only validation of BaSim3Graph.covariance / gate (ba_sim3_cov_check); raises BaError.
    pose_sel: user indices; pairs: (j, k) arrays or (n, 2); candidates: dict(j, k, Z, Omega)."""
    _graph_cov_check("ba_sim3", 7, n_pose, pose_fixed, pose_sel, pairs, candidates)


def sim3_exp(xi):
    """The library's sim3_exp (csrc/ba_sim3_fn.h, on the host): xi = [v; omega; sigma] -> S13"""
    xi, S = np.ascontiguousarray(xi, np.float64).reshape(7), np.zeros(13)
    _lib.load().ba_sim3_exp(_dp(xi), _dp(S))
    return S


def sim3_log(S13):
    """The library's sim3_log (on the host): S13 = [R row-major, t, s] -> xi = [v; omega; sigma]"""
    S, xi = np.ascontiguousarray(S13, np.float64).reshape(13), np.zeros(7)
    _lib.load().ba_sim3_log(_dp(S), _dp(xi))
    return xi


def sim3_adjoint(S13):
    """The library's Ad7 (on the host): [[sR, hat(t) R, -t], [0, R, 0], [0, 0, 1]] (7, 7)"""
    S, Ad = np.ascontiguousarray(S13, np.float64).reshape(13), np.zeros((7, 7))
    _lib.load().ba_sim3_adjoint(_dp(S), _dp(Ad))
    return Ad


class BaSim3Graph(_BaGraph):
    """Sim(3) pose-graph optimisation (ba_sim3_* of include/ba_hip.h): the 7-DoF
    loop closing of a monocular map, chi-square Levenberg-Marquardt over relative-similarity
    factors alone.  pose_S (n, 13) S_jw = [R row-major, t, s] in scaled units, pose_fixed (n,)
    or None, rels = dict(j (F,), k (F,), Z (F, 13), Omega (F, 7, 7)).  The structure is planned
    once; update_values + solve re-optimise new values.  owner: a BaProblem whose handle is
    borrowed, or None for a handle of its own."""

    _abi, _W, _pose_arg = "ba_sim3", 7, "pose_S"
    _info_keys = _BaGraph._info_keys + ("fpb",)

    def __init__(self, pose_S, pose_fixed, rels, device=0, owner=None):
        super().__init__(pose_S, pose_fixed, rels, device, owner)

    def update_values(self, pose_S=None, Z=None, Omega=None):
        """New values for the same structure (ba_sim3_update_values); None keeps."""
        self._update_values(pose_S, Z, Omega)

    def factor_weights(self):
        """-> (s (F,), w (F,)): s_f = r_f^T Omega_f r_f and the robust weight w_f of every factor
        at the poses the object holds (ba_sim3_factor_weights); w = 1 without a kernel"""
        return self._factor_sw("factor_weights")

    def factor_report(self):
        """-> s (F,): s_f = r_f^T Omega_f r_f of every factor at the poses the object holds"""
        s = np.zeros(self.n_rel)
        self._call("factor_report", self.g, _dp(s))
        return s


class BaStream:
    """Observation streaming (include/ba_hip.h ba_stream_*): the
    same problem-construction calls and LM loop as BaProblem for a problem whose
    landmark-side data does not have to fit in device memory — n_chunks landmark
    chunks pass through two device arenas of arena_bytes each, twice per iteration."""

    def __init__(self, device=0, n_chunks=4, arena_bytes=1 << 30):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.ba_stream_create(C.byref(h), device, n_chunks, arena_bytes),
              "ba_stream_create")
        self.h = h
        self.n_pose = self.n_pt = 0

    def close(self):
        if self.h:
            self.lib.ba_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_cameras(self, intr4, T_cj12):
        intr4 = np.ascontiguousarray(intr4, np.float64).reshape(-1, 4)
        T = np.ascontiguousarray(T_cj12, np.float64).reshape(-1, 12)
        check(self.lib.ba_stream_set_cameras(self.h, intr4.shape[0], _dp(intr4), _dp(T)),
              "ba_stream_set_cameras")

    def set_poses(self, T_jw12, fixed):
        T = np.ascontiguousarray(T_jw12, np.float64).reshape(-1, 12)
        f = np.ascontiguousarray(fixed, np.uint8)
        self.n_pose = T.shape[0]
        check(self.lib.ba_stream_set_poses(self.h, T.shape[0], _dp(T), _up(f)),
              "ba_stream_set_poses")

    def set_points(self, X3, fixed):
        X = np.ascontiguousarray(X3, np.float64).reshape(-1, 3)
        f = np.ascontiguousarray(fixed, np.uint8)
        self.n_pt = X.shape[0]
        check(self.lib.ba_stream_set_points(self.h, X.shape[0], _dp(X), _up(f)),
              "ba_stream_set_points")

    def set_observations(self, cam, pose, pt, uv):
        cam = np.ascontiguousarray(cam, np.int32)
        pose = np.ascontiguousarray(pose, np.int32)
        pt = np.ascontiguousarray(pt, np.int32)
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        check(self.lib.ba_stream_set_observations(self.h, cam.shape[0], _ip(cam), _ip(pose),
                                                  _ip(pt), _dp(uv)),
              "ba_stream_set_observations")

    def finalize(self):
        check(self.lib.ba_stream_finalize(self.h), "ba_stream_finalize")

    def solve(self, opt, cap=None):
        cap = cap or max(1, opt.max_num_iterations)
        rows = (BaIterInfo * cap)()
        n = C.c_int(0)
        conv = C.c_int(0)
        check(self.lib.ba_stream_solve(self.h, C.byref(opt), rows, cap, C.byref(n),
                                       C.byref(conv)), "ba_stream_solve")
        return [rows[i] for i in range(min(n.value, cap))], bool(conv.value)

    def lm_begin(self, opt):
        check(self.lib.ba_stream_lm_begin(self.h, C.byref(opt)), "ba_stream_lm_begin")

    def lm_iterate(self, n):
        check(self.lib.ba_stream_lm_iterate(self.h, n), "ba_stream_lm_iterate")

    def lm_sync(self, cap=0):
        rows = (BaIterInfo * max(cap, 1))()
        n = C.c_int(0)
        conv = C.c_int(0)
        rc = check(self.lib.ba_stream_lm_sync(self.h, rows, cap, C.byref(n), C.byref(conv)),
                   "ba_stream_lm_sync")
        return ([rows[i] for i in range(min(n.value, cap))], n.value, bool(conv.value), bool(rc))

    def get_poses(self):
        out = np.zeros((self.n_pose, 12))
        check(self.lib.ba_stream_get_poses(self.h, _dp(out)), "ba_stream_get_poses")
        return out

    def get_points(self):
        out = np.zeros((self.n_pt, 3))
        check(self.lib.ba_stream_get_points(self.h, _dp(out)), "ba_stream_get_points")
        return out

    def info(self):
        v = (C.c_int64 * 6)()
        check(self.lib.ba_stream_info(self.h, v), "ba_stream_info")
        return dict(arena_bytes=v[0], largest_chunk_bytes=v[1], all_chunks_bytes=v[2],
                    bytes_h2d=v[3], bytes_d2h=v[4], n_chunks=v[5])


def _begin_summary(summary, options):
    """the options' thresholds and iteration limit into a Summary (None: nothing)"""
    if summary is not None:
        summary.max_iteration_ = options.iteration_handle.max_num_iterations
        summary.threshold_cost_change_ = options.convergence_handle.threshold_cost_change
        summary.threshold_step_size_ = options.convergence_handle.threshold_step_size
        summary.convergence_status_ = True


# a kind of pose graph as the facade's shared graph methods see it (FullBundleAdjustmentSolver._graph_kind)
_GraphKind = collections.namedtuple("_GraphKind", "cls add rels units poses to_user")


class FullBundleAdjustmentSolver:
    """Mirror of reference core/full_bundle_adjustment_solver.h:127-146.

    Poses are 4x4 numpy arrays (world->camera-body pose, as in
    test/test_ba.cpp:162-167), points 3-vectors.  As in the reference the
    solver identifies them by OBJECT IDENTITY (`id(obj)` plays the role of
    the pointer key) and writes the result back INTO the same arrays at the
    end of Solve.  AddPoseArray / AddPointArray / AddObservations are bulk
    forms (integer handles) for the multi-million-observation configs.
    """

    def __init__(self, device=0, verbose=False):
        self.device = device
        self.verbose = verbose
        self.Reset()
        if self.verbose:
            print("SparseBundleAdjustmentSolver() - initialize.")

    # reference :44-70
    def Reset(self):
        self.camera_id_to_camera_map_ = {}
        self.scaler_ = SCALER
        self.inverse_scaler_ = INVERSE_SCALER
        self._pose_objs = []      # (array, row or None)
        self._pose_key = {}
        self._pose_T_jw = []      # list of (k,12) chunks
        self._pose_fixed = set()
        self._pt_objs = []
        self._pt_key = {}
        self._pt_X = []
        self._pt_fixed = set()
        self._obs_cam, self._obs_pose, self._obs_pt, self._obs_uv = \
            [], [], [], []
        self._relatives = []      # AddRelativePose: one scaled dict (F = 1) per factor, input order
        self._relative_units = []  # per factor: sigma_pixel SCALER, the unit of its Mahalanobis distance
        self._relative_report = None
        self._sim3_relatives = []  # AddRelativeSim3: (j, k, Z13, Omega 7x7) scaled, input order; SolveSim3Graph only
        self._sim3_robust = []     # per Sim(3) factor: (kind, scale in scaled units)
        self._sim3_units = []      # per Sim(3) factor: sigma_pixel SCALER, the unit of its Mahalanobis distance
        self._sim3_report = None
        self.num_total_poses_ = 0
        self.num_total_points_ = 0
        self.num_fixed_poses_ = 0
        self.num_fixed_points_ = 0
        self.num_total_observations_ = 0
        self.num_optimization_poses_ = 0
        self.num_optimization_points_ = 0
        self.is_parameter_finalized_ = False
        self._problem = None
        self._shard = (0, 1)
        self._allreduce = None
        self._stream = None

    # ---- registration ----
    def AddCamera(self, camera_index, camera):          # reference :72-85
        if camera_index in self.camera_id_to_camera_map_:
            return  # unordered_map::insert keeps the first
        c = Camera(camera.fx * SCALER, camera.fy * SCALER, camera.cx * SCALER,
                   camera.cy * SCALER, camera.pose_this_to_cam0)
        c.pose_this_to_cam0[:3, 3] *= SCALER
        self.camera_id_to_camera_map_[camera_index] = c
        if self.verbose:
            print("New camera is added.\n  fx: %g, fy: %g, cx: %g, cy: %g" %
                  (c.fx, c.fy, c.cx, c.cy))

    def _finalized_warning(self):
        sys.stderr.write(_yellow("Cannot enroll parameter. "
                                 "(is_parameter_finalized_ == true)") + "\n")

    def AddPose(self, original_pose):                   # reference :87-101
        if self.is_parameter_finalized_:
            self._finalized_warning()
            return None
        key = id(original_pose)
        if key in self._pose_key:
            return self._pose_key[key]
        T_jw = rigid_inverse(original_pose)
        T_jw[:3, 3] *= SCALER
        h = self.num_total_poses_
        self._pose_key[key] = h
        self._pose_objs.append((original_pose, None))
        self._pose_T_jw.append(_T44_to_12(T_jw))
        self.num_total_poses_ += 1
        return h

    def AddPoseArray(self, poses):
        """Bulk AddPose of an (n,4,4) array; returns integer handles."""
        if self.is_parameter_finalized_:
            self._finalized_warning()
            return None
        poses = np.asarray(poses)
        assert poses.ndim == 3 and poses.shape[1:] == (4, 4) and \
            poses.dtype == np.float64
        T_jw = rigid_inverse(poses)
        T_jw[:, :3, 3] *= SCALER
        base = self.num_total_poses_
        n = poses.shape[0]
        self._pose_objs.extend((poses, r) for r in range(n))
        self._pose_T_jw.append(_T44_to_12(T_jw))
        self.num_total_poses_ += n
        return np.arange(base, base + n, dtype=np.int32)

    def AddPoint(self, original_point):                 # reference :103-117
        if self.is_parameter_finalized_:
            self._finalized_warning()
            return None
        key = id(original_point)
        if key in self._pt_key:
            return self._pt_key[key]
        h = self.num_total_points_
        self._pt_key[key] = h
        self._pt_objs.append((original_point, h, 0))
        self._pt_X.append(np.asarray(original_point, np.float64)
                          .reshape(1, 3) * SCALER)
        self.num_total_points_ += 1
        return h

    def AddPointArray(self, points):
        if self.is_parameter_finalized_:
            self._finalized_warning()
            return None
        points = np.asarray(points)
        assert points.ndim == 2 and points.shape[1] == 3 and \
            points.dtype == np.float64
        base = self.num_total_points_
        n = points.shape[0]
        self._pt_objs.append((points, base, n))
        self._pt_X.append(points * SCALER)
        self.num_total_points_ += n
        return np.arange(base, base + n, dtype=np.int32)

    def _pose_handle(self, pose):
        if isinstance(pose, (int, np.integer)):
            return int(pose) if 0 <= pose < self.num_total_poses_ else None
        return self._pose_key.get(id(pose))

    def _point_handle(self, point):
        if isinstance(point, (int, np.integer)):
            return int(point) if 0 <= point < self.num_total_points_ else None
        return self._pt_key.get(id(point))

    def MakePoseFixed(self, original_pose):             # reference :119-134
        if self.is_parameter_finalized_:
            self._finalized_warning()
            return
        if original_pose is None:
            sys.stderr.write("Empty pointer is conveyed. Skip this one.\n")
            return
        h = self._pose_handle(original_pose)
        if h is None:
            raise RuntimeError("There is no pointer in the BA pose pool.")
        self._pose_fixed.add(h)
        self.num_fixed_poses_ += 1  # counts duplicates too, like the reference

    def MakePointFixed(self, original_point):           # reference :136-153
        if self.is_parameter_finalized_:
            self._finalized_warning()
            return
        if original_point is None:
            sys.stderr.write("Empty pointer is conveyed. Skip this one.\n")
            return
        h = self._point_handle(original_point)
        if h is None:
            raise RuntimeError("There is no pointer in the BA point pool.")
        self._pt_fixed.add(h)
        self.num_fixed_points_ += 1

    def AddObservation(self, camera_index, related_pose, related_point,
                       pixel):                           # reference :155-180
        if camera_index not in self.camera_id_to_camera_map_:
            sys.stderr.write("\033[0;31mInvalid camera index.\n\033[0m")
            return
        hp = self._pose_handle(related_pose)
        if hp is None:
            sys.stderr.write("\033[0;31mNonexisting pose.\n\033[0m")
            return
        hq = self._point_handle(related_point)
        if hq is None:
            sys.stderr.write("\033[0;31mNonexisting point.\n\033[0m")
            return
        self._obs_cam.append(np.array([camera_index], np.int64))
        self._obs_pose.append(np.array([hp], np.int32))
        self._obs_pt.append(np.array([hq], np.int32))
        self._obs_uv.append(np.asarray(pixel, np.float64).reshape(1, 2)
                            * SCALER)
        self.num_total_observations_ += 1

    def AddObservations(self, camera_index, pose_handles, point_handles,
                        pixels):
        """Bulk AddObservation; invalid entries are dropped with a warning,
        as the reference drops them one by one."""
        cam = np.broadcast_to(np.asarray(camera_index, np.int64),
                              np.shape(pose_handles)).copy()
        hp = np.asarray(pose_handles, np.int64)
        hq = np.asarray(point_handles, np.int64)
        uv = np.asarray(pixels, np.float64).reshape(-1, 2)
        known = np.array(sorted(self.camera_id_to_camera_map_), np.int64)
        ok = np.isin(cam, known) & (hp >= 0) & (hp < self.num_total_poses_) \
            & (hq >= 0) & (hq < self.num_total_points_)
        if not ok.all():
            sys.stderr.write("\033[0;31m%d invalid observations dropped.\n"
                             "\033[0m" % int((~ok).sum()))
            cam, hp, hq, uv = cam[ok], hp[ok], hq[ok], uv[ok]
        self._obs_cam.append(cam)
        self._obs_pose.append(hp.astype(np.int32))
        self._obs_pt.append(hq.astype(np.int32))
        self._obs_uv.append(uv * SCALER)
        self.num_total_observations_ += cam.shape[0]

    def AddRelativePose(self, pose_j, pose_k, measurement, information, sigma_pixel=1.0, robust=None):
        """(new) A relative-pose factor between two registered poses (objects or integer
        handles; distinct, not both fixed): an odometry or loop-closure edge of the problem
        that Solve and ComputeCovariance then include (BaProblem.set_relative).  measurement,
        information and sigma_pixel are those of a factor of SolveBatch's `relatives`
        (_scaled_relatives): the measured pose_j^-1 * pose_k in AddPose's convention and
        units, the 6x6 information of the tangent [v; omega] in the caller's units.  Call
        before FinalizeParameters; afterwards it warns and is ignored, as AddPose.
        ReloadParameterValues keeps the factors, Reset drops them.
        robust (default None: none): (kind, scale), a robust kernel for SolvePoseGraph
        (ROBUST_HUBER / ROBUST_CAUCHY / ROBUST_GEMAN_MCCLURE).  scale is the
        Mahalanobis distance c against `information` as given, in the caller's units with
        `sigma_pixel`.  Robust factors are pose-graph only: Solve, SolveBatch and
        ComputeCovariance refuse a factor that carries one."""
        if self.is_parameter_finalized_:
            self._finalized_warning()
            return
        fac = dict(pose_j=pose_j, pose_k=pose_k, measurement=measurement, information=information, robust=robust)
        self._relatives.append(self._scaled_relatives("AddRelativePose", [self], [[fac]], sigma_pixel)[0])
        self._relative_units.append(float(sigma_pixel) * SCALER)

    def _relative_arrays(self):
        """the factors of AddRelativePose as the dict BaProblem.set_relative takes, or None"""
        if not self._relatives:
            return None
        out = {key: np.concatenate([r[key] for r in self._relatives], axis=0) for key in ("j", "k", "Z", "Omega")}
        if any("robust_kind" in r for r in self._relatives):
            for key, dt in (("robust_kind", np.int32), ("robust_scale", np.float64)):
                out[key] = np.concatenate([r.get(key, np.zeros(len(r["j"]), dt)) for r in self._relatives])
        return out

    def ReloadParameterValues(self):
        """(new) Read the CURRENT values of every registered pose / point object again
        and hand them to the finalized problem (ba_update_values): a SLAM back end that
        re-optimises the same graph with new values pays no second FinalizeParameters
        (index assignment, plan, uploads).  The reference keeps its own copies from
        AddPose / AddPoint across Solve calls (:44-70, :87-117) and offers no such call;
        without it this facade, like the reference, continues from its internal state."""
        if not self.is_parameter_finalized_:
            return   # nothing planned yet: FinalizeParameters reads the stored copies
        T = np.zeros((self.num_total_poses_, 12))
        for h, (obj, row) in enumerate(self._pose_objs):
            Tw = np.asarray(obj if row is None else obj[row], np.float64)
            T_jw = rigid_inverse(Tw)
            T_jw[:3, 3] *= SCALER
            T[h] = _T44_to_12(T_jw[None])[0]
        X = np.zeros((self.num_total_points_, 3))
        for obj, base, cnt in self._pt_objs:
            if cnt == 0:
                X[base] = np.asarray(obj, np.float64).reshape(3) * SCALER
            else:
                X[base:base + cnt] = np.asarray(obj, np.float64) * SCALER
        self._problem.update_values(T, X)

    # ---- multi-GPU plumbing (new) ----
    def SetShard(self, rank, world, allreduce=None, stream=None):
        """allreduce: a callable hook(which, dev_ptr, n_doubles, stream) -> int, or
        an exchange object with .attach(problem) (sharding.TorchExchange /
        sharding.RcclExchange built with problem=None)."""
        self._shard = (rank, world)
        self._allreduce = allreduce
        self._stream = stream

    # ---- finalize / solve ----
    def _host_arrays(self):
        """The registered problem as C-ABI level arrays (host only, no GPU)."""
        if not self.camera_id_to_camera_map_ or not self.num_total_poses_ \
                or not self.num_total_points_:
            raise RuntimeError("cameras, poses and points must be added "
                               "before FinalizeParameters")
        cam_ids = sorted(self.camera_id_to_camera_map_)
        cam_pos = {cid: k for k, cid in enumerate(cam_ids)}
        intr = np.array([[c.fx, c.fy, c.cx, c.cy] for c in
                         (self.camera_id_to_camera_map_[i] for i in cam_ids)])
        camT = _T44_to_12(np.stack([self.camera_id_to_camera_map_[i]
                                    .pose_this_to_cam0 for i in cam_ids]))
        T_jw = np.concatenate(self._pose_T_jw, axis=0)
        X = np.concatenate(self._pt_X, axis=0)
        pf = np.zeros(self.num_total_poses_, np.uint8)
        pf[list(self._pose_fixed)] = 1
        qf = np.zeros(self.num_total_points_, np.uint8)
        qf[list(self._pt_fixed)] = 1
        if self._obs_cam:
            cam_raw = np.concatenate(self._obs_cam)
            lut = np.full(int(max(cam_ids)) + 1, -1, np.int64)
            for cid, k in cam_pos.items():
                lut[cid] = k
            ocam = lut[cam_raw].astype(np.int32)
            opose = np.concatenate(self._obs_pose)
            opt = np.concatenate(self._obs_pt)
            ouv = np.concatenate(self._obs_uv, axis=0)
        else:
            ocam = opose = opt = np.zeros(0, np.int32)
            ouv = np.zeros((0, 2))
        return intr, camT, T_jw, X, pf, qf, ocam, opose, opt, ouv

    def FinalizeParameters(self):   # reference :182-206 (private there)
        if self.is_parameter_finalized_:
            return
        refuse_robust("FinalizeParameters", self._relative_arrays())   # before anything is allocated
        intr, camT, T_jw, X, pf, qf, ocam, opose, opt, ouv = self._host_arrays()
        p = BaProblem(self.device)
        p.set_cameras(intr, camT)
        p.set_poses(T_jw, pf)
        p.set_points(X, qf)
        p.set_observations(ocam, opose, opt, ouv)
        if self._shard[1] > 1:
            p.set_shard(*self._shard)
        if self._stream is not None:
            p.set_stream(self._stream)
        if self._relatives:
            if self._allreduce is not None:
                raise _lib.BaError("relative-pose factors (AddRelativePose) run on one GPU; this solver is sharded")
            p.set_relative(self._relative_arrays())   # refuses a factor that carries a robust kernel
        p.finalize()
        if self._allreduce is not None:
            if hasattr(self._allreduce, "attach"):   # an exchange object (sharding.py)
                self._allreduce.attach(p)
            else:                                    # hook(which, ptr, n, stream) -> int
                p.set_allreduce(self._allreduce)
        self._problem = p
        self._connectivity_input = (pf, qf, opose, opt)
        self.num_optimization_poses_ = int((pf == 0).sum())
        self.num_optimization_points_ = int((qf == 0).sum())
        self.is_parameter_finalized_ = True

    def CheckPoseAndPointConnectivity(self):   # reference :310-341
        """stderr warnings for an optimisable pose that observes fewer than 5
        distinct points and for an optimisable point seen from fewer than 2
        distinct poses (fixed ones count, reference :684-693).  Indices are the
        optimisation indices (here: input order of the non-fixed entries; the
        reference's are hash-order)."""
        if self.is_parameter_finalized_:
            pf, qf, opose, opt = self._connectivity_input
        else:
            _, _, _, _, pf, qf, _, opose, opt, _ = self._host_arrays()
        n_pt = max(1, self.num_total_points_)
        pairs = np.unique(opose.astype(np.int64) * n_pt + opt.astype(np.int64))
        pts_of_pose = np.bincount(pairs // n_pt, minlength=self.num_total_poses_)
        poses_of_pt = np.bincount(pairs % n_pt, minlength=self.num_total_points_)
        j_opt = np.cumsum(pf == 0) - 1
        i_opt = np.cumsum(qf == 0) - 1
        for h in np.nonzero((pf == 0) & (pts_of_pose < 5))[0]:
            sys.stderr.write(_yellow(
                "%d-th pose: It might diverge because some frames have "
                "insufficient related points." % j_opt[h]) + "\n")
        for h in np.nonzero((qf == 0) & (poses_of_pt < 2))[0]:
            sys.stderr.write(_yellow(
                "%d-th point: It might diverge because some points have "
                "insufficient related poses." % i_opt[h]) + "\n")

    def GetSolverStatistics(self):   # reference :208-239 (returns "", Q8)
        print("| Bundle Adjustment Statistics:")
        print("| # cameras in rigid body system: %d" %
              len(self.camera_id_to_camera_map_))
        print("|             # of total poses: %d" % self.num_total_poses_)
        print("|               - # fix  poses: %d" % self.num_fixed_poses_)
        print("|               - # opt. poses: %d" %
              self.num_optimization_poses_)
        print("|            # of total points: %d" % self.num_total_points_)
        print("|              - # fix  points: %d" % self.num_fixed_points_)
        print("|              - # opt. points: %d" %
              self.num_optimization_points_)
        print("|            # of observations: %d" %
              self.num_total_observations_)
        print("|                Jacobian size: %d rows x %d cols" %
              (6 * self.num_total_observations_,
               3 * self.num_optimization_points_ +
               6 * self.num_optimization_poses_))
        print("|                Residual size: %d rows\n" %
              (2 * self.num_total_observations_))
        return ""

    def _use_gauss_newton(self, options):
        """FullBundleAdjustmentSolver::Solve ignores options.solver_type and is
        always Levenberg-Marquardt."""
        return False

    def Solve(self, options, summary=None):             # reference :630-1044
        t0 = time.perf_counter()
        _begin_summary(summary, options)
        self.FinalizeParameters()
        if self.verbose:
            self.GetSolverStatistics()
        self.CheckPoseAndPointConnectivity()            # reference :703
        p = self._problem
        c_opt = options.to_c()
        c_opt.gauss_newton = 1 if self._use_gauss_newton(options) else 0
        rows, converged = p.solve(c_opt)
        return self._finish_solve(rows, converged, summary, t0)

    # ---- the two pose graphs: one path, taking the kind ----
    def _graph_kind(self, sim3):
        """What differs between the SE(3) graph of AddRelativePose and the Sim(3) graph of
        AddRelativeSim3, for the shared graph methods below: the graph class, the word in the
        messages, the factor arrays (None: no factor), the factors' units, the registered poses as
        the graph takes them and a covariance block in the caller's units."""
        if sim3:   # (sigma_pixel SCALER)^2 D Sigma D, D = diag(100 I3, I4): the vector d of _scaled_sim3
            d = np.r_[np.full(3, INVERSE_SCALER), np.ones(4)]
            return _GraphKind(BaSim3Graph, "AddRelativeSim3", self._sim3_arrays() if self._sim3_relatives else None,
                              self._sim3_units, lambda T: np.c_[T, np.ones(len(T))],   # the similarity (R, t, s = 1)
                              lambda b, unit: (unit * unit) * (d[None, :, None] * b * d[None, None, :]))
        return _GraphKind(BaPoseGraph, "AddRelativePose", self._relative_arrays(), self._relative_units, lambda T: T,
                          lambda b, unit: covariance_to_user_units(b, np.zeros((0, 3, 3)), unit / SCALER)[0])

    def _graph(self, kind, what):
        """the registered poses and the kind's factors as a graph, robust kernels included (the
        factor dict carries them); needs no FinalizeParameters"""
        if kind.rels is None or not self.num_total_poses_:
            raise RuntimeError("%s: poses (AddPose) and factors (%s) must be added first" % (what, kind.add))
        pf = np.zeros(self.num_total_poses_, np.uint8)
        pf[list(self._pose_fixed)] = 1
        return kind.cls(kind.poses(np.concatenate(self._pose_T_jw, axis=0)), pf, kind.rels, self.device)

    @staticmethod
    def _graph_unit(what, units, more=()):
        """the one unit sigma_pixel SCALER of every factor (and of `more`): Sigma and d2 have
        caller's units only if there is one"""
        units = list(units) + list(more)
        for u in units:
            if u != units[0]:
                raise RuntimeError("%s: the factors and candidates were given with sigma_pixel = %g and %g; "
                                   "a covariance in the caller's units needs one value"
                                   % (what, units[0] / SCALER, u / SCALER))
        return units[0] if units else SCALER

    def _pose_handles(self, objs):
        hs = [self._pose_handle(o) for o in objs]
        if any(h is None for h in hs):
            raise RuntimeError("There is no pointer in the BA pose pool.")
        return np.asarray(hs, np.int32)

    def _solve_graph(self, kind, what, options, report):
        """-> rows, converged, the solved poses and (s in the caller's units, w) of report(graph)"""
        c_opt = options.to_c()
        c_opt.gauss_newton = 1 if self._use_gauss_newton(options) else 0
        with self._graph(kind, what) as g:
            rows, converged = g.solve(c_opt)
            new = g.poses()
            s, w = report(g)
        unit = np.asarray(kind.units)   # s in scaled units = s in the caller's times unit^2
        return rows, converged, new, (s / (unit * unit), w)

    def _graph_covariance(self, kind, what, poses, pairs):
        unit = self._graph_unit(what, kind.units)
        ps = self._pose_handles(poses)
        pj, pk = self._pose_handles([p[0] for p in pairs]), self._pose_handles([p[1] for p in pairs])
        with self._graph(kind, what) as g:
            blocks = g.covariance(ps, (pj, pk))
        return tuple(kind.to_user(b, unit) for b in blocks)

    def _graph_gate(self, kind, what, candidates, scaled):
        """scaled(sig, unit) -> j, k, Z, Omega of the candidates in scaled units, the kind's own
        way; sig: each candidate's sigma_pixel, unit: the one unit of factors and candidates"""
        sig = [float(c.get("sigma_pixel", 1.0)) for c in candidates]
        unit = self._graph_unit(what, kind.units, [v * SCALER for v in sig])
        j, k, Z, Om = scaled(sig, unit)
        with self._graph(kind, what) as g:
            d2 = g.gate(j, k, Z, Om)[0]
        return d2 / (unit * unit)

    @staticmethod
    def _graph_weights(what, solve, report):
        if report is None:
            raise RuntimeError("%s: %s has not run" % (what, solve))
        s, w = report
        return s.copy(), w.copy()

    def SolvePoseGraph(self, options, summary=None):
        """(new) Pose-graph optimisation: Levenberg-Marquardt over the factors of
        AddRelativePose ALONE, on the registered poses with their fixed flags (BaPoseGraph,
        ba_pgraph_*; chi-square LM).  Needs no camera, point, observation or
        FinalizeParameters.  options.solver_type GAUSS_NEWTON is honoured by the refactored
        class as in its Solve.  Fills `summary` from the rows and writes the poses back into
        the registered pose objects as Solve does; the solver's own copies follow, so that a
        second call continues from the first.  A finalized problem of the same solver takes
        the new poses with ReloadParameterValues.  Factors added with robust=(kind, scale) are
        solved with their kernels; GetRelativeWeights returns every factor's
        s and weight at the solved poses."""
        t0 = time.perf_counter()
        _begin_summary(summary, options)
        rows, converged, T_new, self._relative_report = self._solve_graph(
            self._graph_kind(False), "SolvePoseGraph", options, lambda g: g.factor_report())
        self._pose_T_jw = [T_new]
        n_pt = self.num_total_points_
        return self._write_back(T_new, np.zeros((n_pt, 3)), np.zeros(n_pt, bool), rows, converged, summary, t0)

    def GetRelativeWeights(self):
        """(new) -> (s, w) of the last SolvePoseGraph, one entry per factor in the order of
        AddRelativePose, at the solved poses: s = r^T information r in the caller's units
        (the Mahalanobis distance squared that a robust scale is compared with) and the
        robust weight w (1 for a factor without a kernel).  A closure with a small w is the one to drop."""
        return self._graph_weights("GetRelativeWeights", "SolvePoseGraph", self._relative_report)

    def ComputePoseGraphCovariance(self, poses, pairs=()):
        """(new) -> (cov_pose (n, 6, 6), cov_cross (p, 6, 6), cov_rel (p, 6, 6)) of the pose graph
        that SolvePoseGraph solves, at the registered poses as they are now (BaPoseGraph.covariance,
        DESIGN.md §6m; nothing is solved, FinalizeParameters is not needed): the marginal
        covariance of each pose of `poses` (objects or handles, optimisable), and for each
        (pose_j, pose_k) of `pairs` the cross block Sigma_jk and the covariance of the relative
        pose T_jw T_kw^-1.  Caller's units (covariance_to_user_units) for the sigma_pixel the
        factors were added with; factors with different sigma_pixel raise RuntimeError."""
        return self._graph_covariance(self._graph_kind(False), "ComputePoseGraphCovariance", poses, pairs)

    def GateLoopClosures(self, candidates):
        """(new) -> d2 (n,) of loop-closure candidates against the pose graph at the registered
        poses, BEFORE they are added (BaPoseGraph.gate): the squared Mahalanobis
        distance of each candidate's residual under the estimate's own uncertainty plus the
        candidate's, in the caller's units; accept below a chi-square quantile of 6 degrees of
        freedom (22.46 at 0.999).  A candidate is a dict with the keys of AddRelativePose
        (pose_j, pose_k, measurement, information, optionally sigma_pixel = 1.0), and every
        candidate and factor must have been given with one sigma_pixel (RuntimeError otherwise)."""
        def scaled(sig, unit):   # all candidates with the one unit; refuses a candidate that carries a kernel
            facs = [dict(pose_j=c["pose_j"], pose_k=c["pose_k"], measurement=c["measurement"],
                         information=c["information"], robust=c.get("robust")) for c in candidates]
            sr = self._scaled_relatives("GateLoopClosures", [self], [facs], unit / SCALER)[0]
            return sr["j"], sr["k"], sr["Z"], sr["Omega"]
        return self._graph_gate(self._graph_kind(False), "GateLoopClosures", candidates, scaled)

    def AddRelativeSim3(self, pose_j, pose_k, measurement, information, sigma_pixel=1.0, robust=None):
        """(new) A relative-similarity factor between two registered poses (objects or integer
        handles; distinct, not both fixed) for SolveSim3Graph, the 7-DoF loop closing of a
        monocular map.  measurement: a 4x4 similarity [[sR, t], [0, 1]], the
        measured pose_j^-1 * pose_k in AddPose's convention and units (s = 1: a rigid edge).
        information: the 7x7 of the tangent [v; omega; sigma] in the caller's units, scaled as
        _scaled_relatives scales the 6x6 (sigma, like omega, has no unit).  Solve, SolveBatch,
        ComputeCovariance and SolvePoseGraph never see these factors; SolveSim3Graph sees no
        factor of AddRelativePose.  May be called at any time; Reset drops the factors.
        robust (default None: none): (kind, scale) as AddRelativePose takes it, a robust kernel
        for SolveSim3Graph; scale is the Mahalanobis distance c against
        `information` as given, in the caller's units with `sigma_pixel`."""
        hj, hk = self._pose_handle(pose_j), self._pose_handle(pose_k)
        if hj is None or hk is None:
            raise RuntimeError("There is no pointer in the BA pose pool.")
        kind, scale = 0, 0.0
        if robust is not None and int(robust[0]) != 0:
            sim3_robust_check([int(robust[0])], [float(robust[1])])
            # s in scaled units is s in the caller's units times (sigma_pixel SCALER)^2
            kind, scale = int(robust[0]), float(robust[1]) * float(sigma_pixel) * SCALER
        Z, Om = self._scaled_sim3(measurement, information, sigma_pixel)
        self._sim3_relatives.append((hj, hk, Z, Om))
        self._sim3_robust.append((kind, scale))
        self._sim3_units.append(float(sigma_pixel) * SCALER)

    @staticmethod
    def _scaled_sim3(measurement, information, sigma_pixel):
        """a 4x4 similarity and a 7x7 information in the caller's units -> (Z13, Omega 7x7) scaled"""
        M = np.array(measurement, np.float64).reshape(4, 4)
        with np.errstate(all="ignore"):
            s = float(np.cbrt(np.linalg.det(M[:3, :3])))
            Z = np.r_[(M[:3, :3] / s).reshape(9), M[:3, 3] * SCALER, s]
        d = np.r_[np.full(3, INVERSE_SCALER), np.ones(4)]
        w = 1.0 / (float(sigma_pixel) ** 2 * SCALER * SCALER)
        Om = (d[:, None] * np.asarray(information, np.float64).reshape(7, 7) * d[None, :]) / w
        return Z, Om

    def _sim3_arrays(self):
        f = self._sim3_relatives
        out = dict(j=np.array([r[0] for r in f], np.int32), k=np.array([r[1] for r in f], np.int32),
                   Z=np.array([r[2] for r in f]).reshape(-1, 13), Omega=np.array([r[3] for r in f]).reshape(-1, 7, 7))
        if any(kd for kd, _ in self._sim3_robust):   # the kernels the factors carry; none: the dict of before
            out.update(robust_kind=np.array([kd for kd, _ in self._sim3_robust], np.int32),
                       robust_scale=np.array([c for _, c in self._sim3_robust], np.float64))
        return out

    def SolveSim3Graph(self, options, summary=None, point_anchors=None):
        """(new) Sim(3) pose-graph optimisation over the factors of AddRelativeSim3 ALONE, on the
        registered poses with their fixed flags (BaSim3Graph, ba_sim3_*).  Every
        registered pose starts as the similarity (R, t, s = 1) of its rigid pose.  Fills `summary`
        as SolvePoseGraph does and writes each pose back RIGID, T_jw = [R, t / s]; returns the
        scale s per registered pose (1 for a fixed pose).
        point_anchors: None, or one entry per registered point: a registered pose (object or
        handle), or None / a negative handle to leave the point.  An anchored, non-fixed point
        moves to S_new,a^-1 (T_old,a X), so that its projection into its anchor keyframe is
        unchanged.  The solver's own copies follow; a finalized problem of the same solver takes
        poses and points with ReloadParameterValues.  Factors added with robust=(kind, scale) are
        solved with their kernels; GetRelativeSim3Weights returns every factor's s
        and weight at the solved poses."""
        t0 = time.perf_counter()
        _begin_summary(summary, options)
        if not self._sim3_relatives or not self.num_total_poses_:   # before the anchors are looked at, as ever
            raise RuntimeError("SolveSim3Graph: poses (AddPose) and factors (AddRelativeSim3) must be added first")
        n_pt = self.num_total_points_
        anchors = np.full(n_pt, -1, np.int64)
        if point_anchors is not None:
            if len(point_anchors) != n_pt:
                raise ValueError("SolveSim3Graph: one anchor (or None) per registered point")
            for i, a in enumerate(point_anchors):
                if a is None or (isinstance(a, (int, np.integer)) and a < 0):
                    continue
                h = self._pose_handle(a)
                if h is None:
                    raise RuntimeError("There is no pointer in the BA pose pool.")
                anchors[i] = h

        def report(g):
            if any(kd for kd, _ in self._sim3_robust):
                return g.factor_weights()
            s = g.factor_report()   # no kernel: the report of before, nothing robust is allocated or launched
            return s, np.ones(len(s))
        T_old = np.concatenate(self._pose_T_jw, axis=0)
        rows, converged, S_new, self._sim3_report = self._solve_graph(
            self._graph_kind(True), "SolveSim3Graph", options, report)
        scales = S_new[:, 12].copy()
        T_new = S_new[:, :12].copy()
        T_new[:, 9:12] /= scales[:, None]
        X = np.concatenate(self._pt_X, axis=0) if n_pt else np.zeros((0, 3))
        moved = anchors >= 0
        moved[list(self._pt_fixed)] = False
        if moved.any():
            a = anchors[moved]
            Ro, to = T_old[a, :9].reshape(-1, 3, 3), T_old[a, 9:12]
            Rn, tn, sn = S_new[a, :9].reshape(-1, 3, 3), S_new[a, 9:12], scales[a]
            Y = np.einsum("nij,nj->ni", Ro, X[moved]) + to
            X = X.copy()
            X[moved] = np.einsum("nji,nj->ni", Rn, (Y - tn) / sn[:, None])
            self._pt_X = [X]
        self._pose_T_jw = [T_new]
        self._write_back(T_new, X, moved, rows, converged, summary, t0)
        return scales

    def GetRelativeSim3Weights(self):
        """(new) -> (s, w) of the last SolveSim3Graph, one entry per factor in the order of
        AddRelativeSim3, at the solved similarities: s = r^T information r in the caller's units
        and the robust weight w (1 for a factor without a kernel)."""
        return self._graph_weights("GetRelativeSim3Weights", "SolveSim3Graph", self._sim3_report)

    def ComputeSim3GraphCovariance(self, poses, pairs=()):
        """(new) -> (cov_pose (n, 7, 7), cov_cross (p, 7, 7), cov_rel (p, 7, 7)) of the Sim(3) graph
        that SolveSim3Graph solves, at the registered poses as they are now, each the similarity
        (R, t, s = 1) (BaSim3Graph.covariance; nothing is solved): the marginal
        covariance of each pose of `poses` (objects or handles, optimisable) in the tangent
        [v; omega; sigma], and for each (pose_j, pose_k) of `pairs` the cross block Sigma_jk and
        the covariance of S_jw S_kw^-1.  Caller's units for the sigma_pixel the factors were added
        with: (sigma_pixel SCALER)^2 D Sigma D with D = diag(100 I3, I4), the vector d of
        AddRelativeSim3 (omega and sigma have no unit); factors with different sigma_pixel raise
        RuntimeError."""
        return self._graph_covariance(self._graph_kind(True), "ComputeSim3GraphCovariance", poses, pairs)

    def GateSim3LoopClosures(self, candidates):
        """(new) -> d2 (n,) of Sim(3) loop-closure candidates against the Sim(3) graph at the
        registered poses, BEFORE they are added (BaSim3Graph.gate), in the caller's
        units; accept below a chi-square quantile of 7 degrees of freedom (24.32 at 0.999).  A
        candidate is a dict with the keys of AddRelativeSim3 (pose_j, pose_k, measurement,
        information, optionally sigma_pixel = 1.0); every candidate and factor must have been
        given with one sigma_pixel (RuntimeError otherwise).  No robust weight applies to a candidate."""
        def scaled(sig, unit):   # each candidate with its own sigma_pixel (the factors'); its kernel is not read
            hj = self._pose_handles([c["pose_j"] for c in candidates])
            hk = self._pose_handles([c["pose_k"] for c in candidates])
            zo = [self._scaled_sim3(c["measurement"], c["information"], sg) for c, sg in zip(candidates, sig)]
            return hj, hk, np.array([z for z, _ in zo]).reshape(-1, 13), np.array([om for _, om in zo]).reshape(-1, 7, 7)
        return self._graph_gate(self._graph_kind(True), "GateSim3LoopClosures", candidates, scaled)

    @staticmethod
    def _scaled_priors(what, solvers, priors, sigma_pixel):
        """priors of SolveBatch / ComputeCovarianceBatch / MarginalizeBatch -> the list
        BaBatch.set_prior takes (scaled units), or None.  priors[k]: None, or a dict with
        poses (pose objects or handles, optimisable; sorted here into registration order
        together with the blocks of H and b), H and b (units of MarginalizeBatch for
        `sigma_pixel`), lin_poses (one per pose, the convention of AddPose, converted as
        AddPose converts) and c (default 0)."""
        if priors is None:
            return None
        if len(priors) != len(solvers):
            raise ValueError("%s: one prior (or None) per solver" % what)
        out = []
        for sv, pr in zip(solvers, priors):
            if pr is None:
                out.append(None)
                continue
            hs = []
            for pose in pr["poses"]:
                h = sv._pose_handle(pose)
                if h is None:
                    raise RuntimeError("There is no pointer in the BA pose pool.")
                hs.append(h)
            K = len(hs)
            order = np.argsort(np.asarray(hs, np.int64), kind="stable")
            cols = (6 * order[:, None] + np.arange(6)[None, :]).reshape(-1)
            H, b, c = prior_to_scaled_units(np.asarray(pr["H"], np.float64).reshape(6 * K, 6 * K),
                                            np.asarray(pr["b"], np.float64).reshape(6 * K),
                                            pr.get("c", 0.0), sigma_pixel)
            T_lin = rigid_inverse(np.asarray(pr["lin_poses"], np.float64).reshape(K, 4, 4))
            T_lin[:, :3, 3] *= SCALER
            out.append(dict(poses=np.asarray(hs, np.int32)[order], H=H[np.ix_(cols, cols)], b=b[cols],
                            T_lin=_T44_to_12(T_lin)[order], c=c))
        return out

    @staticmethod
    def _scaled_relatives(what, solvers, relatives, sigma_pixel):
        """relatives of SolveBatch / ComputeCovarianceBatch / MarginalizeBatch -> the list
        BaBatch.set_relative takes (scaled units), or None.  relatives[k]: None, or a list of
        factors of solver k, each a dict with
          pose_j, pose_k  two registered poses (objects or integer handles), distinct, not
                          both fixed,
          measurement     (4, 4) the measured pose_j^-1 * pose_k in the convention and units
                          of AddPose (T_jw T_kw^-1 after AddPose's conversion),
          information     (6, 6) of the tangent [v; omega] of the world-to-body poses in the
                          caller's units, the units MarginalizeBatch returns for `sigma_pixel`
                          (converted as prior_to_scaled_units converts a 6x6 H).
        A factor with robust=(kind, scale), kind not 0, is taken by AddRelativePose alone
        (s in scaled units is s in the caller's units times (sigma_pixel SCALER)^2, so the
        scale goes in times sigma_pixel SCALER); every other caller refuses it: robust factors
        are pose-graph only."""
        if relatives is None:
            return None
        if len(relatives) != len(solvers):
            raise ValueError("%s: one list of relative-pose factors (or None) per solver" % what)
        out = []
        for sv, fs in zip(solvers, relatives):
            if fs is None:
                out.append(None)
                continue
            j, k = [], []
            Z, Om = np.zeros((len(fs), 12)), np.zeros((len(fs), 6, 6))
            kind, scale = np.zeros(len(fs), np.int32), np.zeros(len(fs))
            for f, fac in enumerate(fs):
                rb = fac.get("robust")
                if rb is not None and int(rb[0]) != 0:
                    if what != "AddRelativePose":
                        raise _lib.BaError("%s: factor %d carries a robust kernel; robust factors are pose-graph "
                                           "only (AddRelativePose + SolvePoseGraph)" % (what, f))
                    pgraph_robust_check([int(rb[0])], [float(rb[1])])
                    kind[f], scale[f] = int(rb[0]), float(rb[1]) * float(sigma_pixel) * SCALER
                hj, hk = sv._pose_handle(fac["pose_j"]), sv._pose_handle(fac["pose_k"])
                if hj is None or hk is None:
                    raise RuntimeError("There is no pointer in the BA pose pool.")
                j.append(hj)
                k.append(hk)
                M = np.array(fac["measurement"], np.float64).reshape(1, 4, 4)
                M[:, :3, 3] *= SCALER
                Z[f] = _T44_to_12(M)[0]
                Om[f] = prior_to_scaled_units(np.asarray(fac["information"], np.float64).reshape(6, 6),
                                              np.zeros(6), 0.0, sigma_pixel)[0]
            out.append(dict(j=np.asarray(j, np.int32), k=np.asarray(k, np.int32), Z=Z, Omega=Om))
            if kind.any():
                out[-1].update(robust_kind=kind, robust_scale=scale)
        return out

    @staticmethod
    def _obs_masks(what, solvers, probs, obs_masks):
        """obs_masks of SolveBatch / ComputeCovarianceBatch / MarginalizeBatch -> one bool array
        per solver (all True for a None entry), or None.  obs_masks[k]: one flag per observation
        solver k registered, in registration order; non-zero = the observation takes part."""
        if obs_masks is None:
            return None
        if len(obs_masks) != len(solvers):
            raise ValueError("%s: one observation mask (or None) per solver" % what)
        out = []
        for k, (pr, m) in enumerate(zip(probs, obs_masks)):
            n = len(pr["obs_pt"])
            if m is None:
                out.append(np.ones(n, bool))
                continue
            m = np.asarray(m).reshape(-1) != 0
            if m.shape[0] != n:
                raise ValueError("%s: solver %d registered %d observations, its mask holds %d flags"
                                 % (what, k, n, m.shape[0]))
            out.append(m)
        return out

    @staticmethod
    def SolveBatch(solvers, options, summaries=None, priors=None, sigma_pixel=1.0, relatives=None,
                   obs_masks=None, cull=None):
        """Solve the registered problems of several solver objects in ONE launch
        (ba_batch_solve: one persistent workgroup per problem, see BaBatch for the
        limits), write every solver's poses and points back as Solve does and fill
        one Summary each (summaries: a list as long as `solvers`, or None).  Returns
        the per-problem BaBatchResult list; a problem whose status is not 0 (over a
        limit, non-finite input) is left untouched.  priors (default None: none):
        one pose prior per solver taken in as one more factor (BaBatch.set_prior), see
        _scaled_priors for the dict; H and b in the units MarginalizeBatch returns for
        `sigma_pixel`.  relatives (default None: none): one list of relative-pose factors
        per solver (BaBatch.set_relative), see _scaled_relatives for the dict.
        obs_masks (default None: none): one flag array per solver (or None), one flag per
        registered observation in registration order; an observation whose flag is 0 takes
        no part (BaBatch.set_obs_mask).  cull (default None: none): a CullOptions; the
        batch is solved with cull.first, every observation with a squared error above
        cull.chi2 * sigma_pixel^2 px^2 (or behind its camera) is switched off, and the
        batch is solved again with `options`, all in one go (BaBatch.solve_culled).  The
        return value is then (results, reports): reports[k] = dict(inliers (bool per
        registered observation: hand it on as obs_masks of ComputeCovarianceBatch and
        MarginalizeBatch), n_culled, starved, n_iter_first); the Summary rows are those of
        both stages."""
        t0 = time.perf_counter()
        solvers = list(solvers)
        if not solvers:
            return []
        if summaries is not None and len(summaries) != len(solvers):
            raise ValueError("SolveBatch: one Summary per solver")
        if any(sv._shard[1] > 1 or sv._allreduce is not None for sv in solvers):
            raise RuntimeError("SolveBatch: a solver with a shard or an all-reduce "
                               "configured cannot be part of a batch")
        probs = []
        for sv in solvers:
            intr, camT, T_jw, X, pf, qf, ocam, opose, opt, ouv = sv._host_arrays()
            probs.append(dict(cam_intr=intr, cam_T=camT, pose_T=T_jw, pose_fixed=pf, pt_X=X,
                              pt_fixed=qf, obs_cam=ocam, obs_pose=opose, obs_pt=opt, obs_uv=ouv))
            sv.CheckPoseAndPointConnectivity()
        c_opt = options.to_c()
        c_opt.gauss_newton = 1 if solvers[0]._use_gauss_newton(options) else 0
        sp = FullBundleAdjustmentSolver._scaled_priors("SolveBatch", solvers, priors, sigma_pixel)
        sr = FullBundleAdjustmentSolver._scaled_relatives("SolveBatch", solvers, relatives, sigma_pixel)
        om = FullBundleAdjustmentSolver._obs_masks("SolveBatch", solvers, probs, obs_masks)
        if cull is not None:
            c_first = cull.first.to_c()
            c_first.gauss_newton = 1 if solvers[0]._use_gauss_newton(cull.first) else 0
            e2_max = cull.e2_max_scaled(sigma_pixel)
            BaBatch.cull_options(e2_max, cull.cull_behind)
            BaBatch.solve_culled_cap(c_first, c_opt)
        batch = BaBatch(probs, solvers[0].device)
        try:
            if sp is not None:
                batch.set_prior(sp)
            if sr is not None:
                batch.set_relative(sr)
            if om is not None:
                batch.set_obs_mask(om)
            reports = None
            if cull is None:
                rows, res = batch.solve(c_opt)
            else:
                rows1, res1, rows, res, cres = batch.solve_culled(c_first, c_opt, e2_max, cull.cull_behind)
                rows = [a + b for a, b in zip(rows1, rows)]
                inl = batch.get_obs_mask()
                reports = [dict(inliers=inl[k].copy(), n_culled=int(cres[k].n_culled),
                                starved=int(cres[k].starved), n_iter_first=int(res1[k].n_iter))
                           for k in range(len(solvers))]
            T_all, X_all = batch.get_poses(), batch.get_points()
            for k, sv in enumerate(solvers):
                summary = None if summaries is None else summaries[k]
                _begin_summary(summary, options)
                if res[k].status != 0:
                    if summary is not None:
                        summary.convergence_status_ = False
                    continue
                T_k, X_k = batch.poses_of(k, T_all).copy(), batch.points_of(k, X_all).copy()
                sv._write_back(T_k, X_k, np.ones(X_k.shape[0], bool), rows[k],
                               bool(res[k].converged), summary, t0)
                # the registered values follow the solution, as after Solve
                sv._pose_T_jw = [T_k]
                sv._pt_X = [X_k]
                if sv._problem is not None:
                    sv._problem.update_values(sv._pose_T_jw[0], sv._pt_X[0])
        finally:
            batch.close()
        return res if reports is None else (res, reports)

    @staticmethod
    def ComputeCovarianceBatch(solvers, sigma_pixel=1.0, options=None, points=True, priors=None,
                               relatives=None, obs_masks=None):
        """(new) Covariance blocks of the CURRENT registered values of several
        solver objects in ONE launch (ba_batch_covariance; see BaBatch for the
        limits).  Returns one (cov_pose (n_pose, 6, 6), cov_point (n_pt, 3, 3) or
        None, BaBatchCovResult) per solver: ALL poses and points in registration
        order, the blocks of fixed members zero, units and conventions those of
        ComputeCovariance.  A result whose status is not 0 (over a limit,
        non-finite input) has zero blocks; dropped_pivots > 0 means S was singular.
        priors: as in SolveBatch; the covariance then includes the past.  relatives: as
        in SolveBatch; every factor joins.  obs_masks: as in SolveBatch (the `inliers` it
        reports): observations that are off take no part."""
        solvers = list(solvers)
        if not solvers:
            return []
        if any(sv._shard[1] > 1 or sv._allreduce is not None for sv in solvers):
            raise RuntimeError("ComputeCovarianceBatch: a solver with a shard or an "
                               "all-reduce configured cannot be part of a batch")
        probs = []
        for sv in solvers:
            intr, camT, T_jw, X, pf, qf, ocam, opose, opt, ouv = sv._host_arrays()
            probs.append(dict(cam_intr=intr, cam_T=camT, pose_T=T_jw, pose_fixed=pf, pt_X=X,
                              pt_fixed=qf, obs_cam=ocam, obs_pose=opose, obs_pt=opt, obs_uv=ouv))
        huber = (options or Options()).outlier_handle.threshold_huber_loss
        sp = FullBundleAdjustmentSolver._scaled_priors("ComputeCovarianceBatch", solvers, priors, sigma_pixel)
        sr = FullBundleAdjustmentSolver._scaled_relatives("ComputeCovarianceBatch", solvers, relatives,
                                                          sigma_pixel)
        om = FullBundleAdjustmentSolver._obs_masks("ComputeCovarianceBatch", solvers, probs, obs_masks)
        batch = BaBatch(probs, solvers[0].device)
        try:
            if sp is not None:
                batch.set_prior(sp)
            if sr is not None:
                batch.set_relative(sr)
            if om is not None:
                batch.set_obs_mask(om)
            cp, cq, res = batch.covariance(huber, points)
            out = []
            for k in range(len(solvers)):
                cp_k = batch.cov_poses_of(k, cp)
                cq_k = batch.cov_points_of(k, cq) if points else np.zeros((0, 3, 3))
                up, uq = covariance_to_user_units(cp_k, cq_k, sigma_pixel)
                out.append((up, uq if points else None, res[k]))
        finally:
            batch.close()
        return out

    @staticmethod
    def MarginalizeBatch(solvers, marg_poses, sigma_pixel=1.0, options=None, priors=None, relatives=None,
                         obs_masks=None):
        """(new) Marginalisation priors of several solver objects in ONE launch
        (ba_batch_marginalize; see BaBatch for the limits), at the CURRENT registered
        values.  marg_poses[k]: the pose objects (or integer handles) of solver k that
        leave its window; the landmarks they observe leave with them.  Returns per
        solver (H (6K, 6K), b (6K,), kept pose handles, marginalised point handles,
        BaBatchMargResult): the Gaussian 1/2 d^T H d - b^T d left on the K kept
        (optimisable, unmarked) poses in registration order, d the stacked tangents
        xi = [v; omega] of the WORLD-TO-BODY poses as in ComputeCovariance, in the
        caller's units for an isotropic pixel noise of `sigma_pixel`
        (marginal_to_user_units).  H is singular where the gauge is free.  A result
        whose status is not 0 is zero; dropped_pivots > 0 means the marked block
        was singular and the prior meaningless.  priors: as in SolveBatch; the old
        prior joins the factors, so priors chain from window to window (the returned b is
        at the current values, which are the lin_poses of the next prior).  relatives: as
        in SolveBatch; a factor joins exactly when one of its two poses is marked and then
        leaves with it, and every tuple gains a sixth entry: one 0 / 1 per factor of that
        solver, 1 where it left (the others go into the next window with the prior).
        obs_masks: as in SolveBatch; the landmarks that leave are those the marked poses
        observe through observations that are on."""
        solvers = list(solvers)
        if not solvers:
            return []
        if len(marg_poses) != len(solvers):
            raise ValueError("MarginalizeBatch: one list of poses per solver")
        if any(sv._shard[1] > 1 or sv._allreduce is not None for sv in solvers):
            raise RuntimeError("MarginalizeBatch: a solver with a shard or an "
                               "all-reduce configured cannot be part of a batch")
        probs, marks = [], []
        for sv, poses in zip(solvers, marg_poses):
            intr, camT, T_jw, X, pf, qf, ocam, opose, opt, ouv = sv._host_arrays()
            probs.append(dict(cam_intr=intr, cam_T=camT, pose_T=T_jw, pose_fixed=pf, pt_X=X,
                              pt_fixed=qf, obs_cam=ocam, obs_pose=opose, obs_pt=opt, obs_uv=ouv))
            mk = np.zeros(len(pf), np.uint8)
            for pose in poses:
                h = sv._pose_handle(pose)
                if h is None:
                    raise RuntimeError("There is no pointer in the BA pose pool.")
                mk[h] = 1
            marks.append(mk)
        huber = (options or Options()).outlier_handle.threshold_huber_loss
        sp = FullBundleAdjustmentSolver._scaled_priors("MarginalizeBatch", solvers, priors, sigma_pixel)
        sr = FullBundleAdjustmentSolver._scaled_relatives("MarginalizeBatch", solvers, relatives, sigma_pixel)
        om = FullBundleAdjustmentSolver._obs_masks("MarginalizeBatch", solvers, probs, obs_masks)
        batch = BaBatch(probs, solvers[0].device)
        try:
            if om is not None:
                batch.set_obs_mask(om)
            if sp is not None:
                batch.set_prior(sp)
            if sr is not None:
                batch.set_relative(sr)
                left = batch.relative_marg_plan(np.concatenate(marks))
                roff = np.concatenate([[0], np.cumsum([0 if r is None else len(r["j"]) for r in sr])])
            Hl, bl, kl, res = batch.marginalize(np.concatenate(marks), huber)
            out = []
            for k in range(len(solvers)):
                Hu, bu = marginal_to_user_units(Hl[k], bl[k], sigma_pixel)
                mq = np.flatnonzero(batch.points_of(k, batch.marg_pt))
                out.append((Hu, bu, [int(h) for h in kl[k]], [int(h) for h in mq], res[k]))
                if sr is not None:
                    out[-1] += ([int(v) for v in left[roff[k]:roff[k + 1]]],)
        finally:
            batch.close()
        return out

    def ComputeCovariance(self, poses, points, sigma_pixel=1.0, options=None):
        """(new; the reference has no counterpart) Covariance blocks of the CURRENT
        solver state — after Solve: of the solution — for the given pose and point
        objects (or integer handles), all optimisable, in any order, repeats allowed.

        Returns (cov_pose (n, 6, 6), cov_point (n, 3, 3)) in the caller's units for an
        isotropic pixel noise of `sigma_pixel`: blocks of sigma^2 (J^T W J)^-1, W the
        Huber weights of `options` (default Options()).  A pose block is the
        covariance of the tangent xi = [v; omega] of the WORLD-TO-BODY pose
        T_jw = inverse(registered pose), left-multiplicative: T_jw <- exp(xi) T_jw,
        v in the caller's length unit, omega in radians.  A point block is the
        covariance of the world point.  Stereo: the solver's own normal matrix is
        inverted (last-writer rule of the cross block, see include/ba_hip.h)."""
        self.FinalizeParameters()
        hp, hq = [], []
        for pose in poses:
            h = self._pose_handle(pose)
            if h is None:
                raise RuntimeError("There is no pointer in the BA pose pool.")
            if h in self._pose_fixed:
                raise RuntimeError("ComputeCovariance: a fixed pose has no covariance.")
            hp.append(h)
        for point in points:
            h = self._point_handle(point)
            if h is None:
                raise RuntimeError("There is no pointer in the BA point pool.")
            if h in self._pt_fixed:
                raise RuntimeError("ComputeCovariance: a fixed point has no covariance.")
            hq.append(h)
        huber = (options or Options()).outlier_handle.threshold_huber_loss
        cp, cq, _ = self._problem.covariance(hp, hq, huber)
        return covariance_to_user_units(cp, cq, sigma_pixel)

    def SolvePointsOnly(self, options, triangulate=()):
        """(new; the reference has no counterpart) Structure-only solve: every registered
        pose is treated as FIXED and every non-fixed registered point is solved on its own
        against its observations, all in one launch (ba_point_only).  triangulate: point
        objects or integer handles whose current value is replaced by a linear
        triangulation first (it may be anything, NaN included).  The current values of
        the solver are used (after Solve: the solution), units are converted as Solve
        does, the new points are written back through the user's objects and become the
        solver's values.  Returns the per-point results (ba_point_result fields) of the
        non-fixed points in registration order; a point whose status is not 0 is left
        as it was."""
        intr, camT, T_jw, X, pf, qf, ocam, opose, opt, ouv = self._host_arrays()
        if self._shard[1] > 1:
            raise RuntimeError("SolvePointsOnly: not available on a sharded solver")
        p = self._problem
        tmp = None
        if p is not None:           # continue from the solver's state, as Solve does
            T_jw, X = p.get_poses(), p.get_points()[0]
        else:
            p = tmp = BaProblem(self.device)
        try:
            sel = np.nonzero(qf == 0)[0]
            tri_all = np.zeros(self.num_total_points_, np.uint8)
            for point in triangulate:
                h = self._point_handle(point)
                if h is None:
                    raise RuntimeError("There is no pointer in the BA point pool.")
                if h in self._pt_fixed:
                    raise RuntimeError("SolvePointsOnly: a fixed point is not triangulated.")
                tri_all[h] = 1
            if sel.size == 0:
                return np.zeros(0, np.dtype(BaPointResult)).view(np.recarray)
            new_of = np.full(self.num_total_points_, -1, np.int64)
            new_of[sel] = np.arange(sel.size)
            keep = new_of[opt] >= 0
            c_opt = options.to_c()
            c_opt.gauss_newton = 1 if self._use_gauss_newton(options) else 0
            Xs, res, _ = point_only(p, intr, camT, T_jw, X[sel], ocam[keep], opose[keep],
                                    new_of[opt[keep]], ouv[keep], c_opt,
                                    triangulate=tri_all[sel], cap=0)
            X = X.copy()
            done = res.status == 0
            X[sel[done]] = Xs[done]
            owned = np.zeros(self.num_total_points_, bool)
            owned[sel[done]] = True
            self._write_points(X, owned)     # no pose is touched
            # the solver's values follow what the user now holds (the value a fresh
            # solver would register from the written point), as after SolveBatch
            X[sel[done]] = (X[sel[done]] * INVERSE_SCALER) * SCALER
            self._pose_T_jw = [np.ascontiguousarray(T_jw)]
            self._pt_X = [X]
            if self._problem is not None:
                self._problem.update_values(None, X)
            return res
        finally:
            if tmp is not None:
                tmp.close()

    def _finish_solve(self, rows, converged, summary, t0):
        """Write the solution back through the user's objects (reference
        :1011-1022) and fill the Summary rows; shared by Solve and
        FullBundleAdjustmentSolverRefactor.SolveByGradientDescent."""
        p = self._problem
        T_jw = p.get_poses()
        if self._shard[1] > 1 and self._allreduce is not None:
            # every rank writes back EVERY point (reference :1018-1022): one final
            # sum-all-reduce of the owned rows
            p.gather_points()
        X, owned = p.get_points()
        return self._write_back(T_jw, X, owned, rows, converged, summary, t0)

    def _write_points(self, X, owned):
        """X [n_pt, 3] (scaled units) into the user's point objects: the non-fixed
        points among `owned`."""
        Xu = X * INVERSE_SCALER
        opt_mask = np.ones(self.num_total_points_, bool)
        opt_mask[list(self._pt_fixed)] = False
        opt_mask &= owned
        for obj, base, cnt in self._pt_objs:
            if cnt == 0:      # single AddPoint object
                if opt_mask[base]:
                    obj[...] = Xu[base].reshape(np.shape(obj))
            else:             # AddPointArray block
                m = opt_mask[base:base + cnt]
                obj[m] = Xu[base:base + cnt][m]

    def _write_back(self, T_jw, X, owned, rows, converged, summary, t0):
        """The second half of _finish_solve on given arrays (scaled units): T_jw
        [n_pose, 12], X [n_pt, 3], owned = the points this rank may write."""
        T44 = _T12_to_44(T_jw)
        T44[:, :3, 3] *= INVERSE_SCALER
        T_wj = rigid_inverse(T44)
        for h, (obj, row) in enumerate(self._pose_objs):
            if h in self._pose_fixed:
                continue
            if row is None:
                obj[...] = T_wj[h]
            else:
                obj[row] = T_wj[h]
        self._write_points(X, owned)
        if summary is not None:
            for r in rows:
                info = OptimizationInfo()
                info.cost = r.cost
                info.cost_change = r.cost_change
                info.average_reprojection_error = r.average_reprojection_error
                info.abs_gradient = r.abs_gradient
                info.abs_step = r.abs_step
                info.damping_term = r.damping_term
                info.iter_time = r.iter_time_ms
                info.iteration_status = IterationStatus(r.iteration_status)
                info.rho, info.model_change, info.trial_cost = \
                    r.rho, r.model_change, r.trial_cost
                summary.optimization_info_list_.append(info)
            summary.convergence_status_ = converged
            summary.total_time_in_millisecond_ = \
                (time.perf_counter() - t0) * 1e3
        return True   # the reference always returns true (:1043)


class PoseOnlyBundleAdjustmentSolver:
    """Mirror of reference core/pose_only_bundle_adjustment_solver.h:25-67
    (monocular and stereo, 6-DoF and planar 3-DoF entry points)."""

    def __init__(self, device=0):
        self._p = BaProblem(device)
        self.debug_poses_ = []

    def GetDebugPoses(self):
        return self.debug_poses_

    def Solve_Monocular_6Dof(self, reference_position_list, matched_pixel_list,
                             fx, fy, cx, cy, reference_to_current_pose,
                             mask_inlier, options, summary=None):
        """reference core/pose_only_bundle_adjustment_solver.cpp:8-170.
        `reference_to_current_pose` is a 4x4 float array updated in place;
        `mask_inlier` a list/array resized to n (True) and updated in place.
        """
        t0 = time.perf_counter()
        X = np.asarray(reference_position_list, np.float32).reshape(-1, 3)
        uv = np.asarray(matched_pixel_list, np.float32).reshape(-1, 2)
        if X.shape[0] != uv.shape[0]:
            raise RuntimeError(
                "In PoseOnlyBundleAdjustmentSolver::"
                "SolveMonocularPoseOnlyBundleAdjustment6Dof(), "
                "world_position_list.size() != current_pixel_list.size()")
        n = X.shape[0]
        if summary is not None:
            summary.max_iteration_ = options.iteration_handle.max_num_iterations
            summary.threshold_cost_change_ = \
                options.convergence_handle.threshold_cost_change
            summary.threshold_step_size_ = \
                options.convergence_handle.threshold_step_size
            summary.convergence_status_ = True
        m = np.ones(n, np.uint8)
        k = min(len(mask_inlier), n)
        m[:k] = np.asarray(mask_inlier[:k], np.uint8)
        T12 = _T44_to_12(np.asarray(reference_to_current_pose,
                                    np.float64)).astype(np.float32)
        res = self._p.pose_only_mono6(X, uv, fx, fy, cx, cy, T12, m,
                                      options.to_c(), want_debug=True)
        self.debug_poses_ = [_T12_to_44(d)[0] for d in res["debug"]]
        if isinstance(mask_inlier, list):
            mask_inlier[:] = [bool(v) for v in res["mask"]]
        else:
            mask_inlier[...] = res["mask"]
        if res["success"]:
            reference_to_current_pose[...] = _T12_to_44(res["T12"])[0]
        if summary is not None:
            for cost, dchg, step in res["rows"]:
                info = OptimizationInfo()
                info.cost = cost
                info.cost_change = abs(dchg)
                info.average_reprojection_error = cost
                info.abs_step = step
                info.abs_gradient = 0
                info.damping_term = -1
                info.iter_time = 0.0
                info.iteration_status = IterationStatus.UPDATE
                summary.optimization_info_list_.append(info)
            summary.convergence_status_ = res["converged"]
            summary.total_time_in_millisecond_ = \
                (time.perf_counter() - t0) * 1e3
        return res["success"]

    def Solve_Stereo_6Dof(self, reference_position_list, matched_left_pixel_list,
                          matched_right_pixel_list, fx_left, fy_left, cx_left,
                          cy_left, fx_right, fy_right, cx_right, cy_right,
                          left_to_right_pose, reference_to_current_left_pose,
                          mask_inlier_left, mask_inlier_right, options,
                          summary=None):
        """reference core/pose_only_bundle_adjustment_solver.cpp:172-399.
        Poses are 4x4 arrays (the left pose is updated in place), the masks
        lists/arrays resized to n (True) and updated in place; a right pixel
        with a negative coordinate means "not matched in the right image"."""
        t0 = time.perf_counter()
        X = np.asarray(reference_position_list, np.float32).reshape(-1, 3)
        ul = np.asarray(matched_left_pixel_list, np.float32).reshape(-1, 2)
        ur = np.asarray(matched_right_pixel_list, np.float32).reshape(-1, 2)
        n = X.shape[0]
        if summary is not None:
            summary.max_iteration_ = options.iteration_handle.max_num_iterations
            summary.threshold_cost_change_ = \
                options.convergence_handle.threshold_cost_change
            summary.threshold_step_size_ = \
                options.convergence_handle.threshold_step_size
            summary.convergence_status_ = True

        def fit(mask):
            m = np.ones(n, np.uint8)
            k = min(len(mask), n)
            m[:k] = np.asarray(mask[:k], np.uint8)
            return m

        to12 = lambda T: _T44_to_12(np.asarray(T, np.float64)).astype(np.float32)
        res = self._p.pose_only_stereo6(
            X, ul, ur, [fx_left, fy_left, cx_left, cy_left],
            [fx_right, fy_right, cx_right, cy_right], to12(left_to_right_pose),
            to12(reference_to_current_left_pose), fit(mask_inlier_left),
            fit(mask_inlier_right), options.to_c(), want_debug=True)
        self.debug_poses_ = [_T12_to_44(d)[0] for d in res["debug"]]
        for mask, key in ((mask_inlier_left, "mask_l"), (mask_inlier_right, "mask_r")):
            if isinstance(mask, list):
                mask[:] = [bool(v) for v in res[key]]
            else:
                mask[...] = res[key]
        if res["success"]:
            reference_to_current_left_pose[...] = _T12_to_44(res["T12"])[0]
        if summary is not None:
            for cost, dchg, step in res["rows"]:
                info = OptimizationInfo()
                info.cost = cost
                info.cost_change = abs(dchg)
                info.average_reprojection_error = cost
                info.abs_step = step
                info.abs_gradient = 0
                info.damping_term = -1
                info.iter_time = 0.0
                info.iteration_status = IterationStatus.UPDATE
                summary.optimization_info_list_.append(info)
            summary.convergence_status_ = res["converged"]
            summary.total_time_in_millisecond_ = \
                (time.perf_counter() - t0) * 1e3
        return res["success"]


    def _finish_pose_only(self, res, pose, masks, summary, t0):
        """Debug poses, masks, pose write-back and Summary rows of a pose-only
        solve, as the 6-DoF methods above do them."""
        self.debug_poses_ = [_T12_to_44(d)[0] for d in res["debug"]]
        for mask, key in masks:
            if isinstance(mask, list):
                mask[:] = [bool(v) for v in res[key]]
            else:
                mask[...] = res[key]
        if res["success"]:
            pose[...] = _T12_to_44(res["T12"])[0]
        if summary is not None:
            for cost, dchg, step in res["rows"]:
                info = OptimizationInfo()
                info.cost = cost
                info.cost_change = abs(dchg)
                info.average_reprojection_error = cost
                info.abs_step = step
                info.abs_gradient = 0
                info.damping_term = -1
                info.iter_time = 0.0
                info.iteration_status = IterationStatus.UPDATE
                summary.optimization_info_list_.append(info)
            summary.convergence_status_ = res["converged"]
            summary.total_time_in_millisecond_ = \
                (time.perf_counter() - t0) * 1e3
        return res["success"]

    @staticmethod
    def _begin_summary(options, summary):
        if summary is not None:     # reference :419-424
            summary.max_iteration_ = options.iteration_handle.max_num_iterations
            summary.threshold_cost_change_ = \
                options.convergence_handle.threshold_cost_change
            summary.threshold_step_size_ = \
                options.convergence_handle.threshold_step_size
            summary.convergence_status_ = True

    @staticmethod
    def _fit_mask(mask, n):
        m = np.ones(n, np.uint8)    # resize(n, true): earlier values kept
        k = min(len(mask), n)
        m[:k] = np.asarray(mask[:k], np.uint8)
        return m

    def _solve_batch(self, frames, options, stereo, planar=False):
        """The batch mirror methods: 6-DoF, or planar 3-DoF (the frames then
        carry the planar methods' parameter names)."""
        t0 = time.perf_counter()
        f32 = lambda a, k: np.asarray(a, np.float32).reshape(-1, k)
        to12 = lambda T: _T44_to_12(np.asarray(T, np.float64)).astype(np.float32)
        xkey = "world_position_list" if planar else "reference_position_list"
        prep = []
        for fr in frames:        # every size check before any device use
            X = f32(fr[xkey], 3)
            if stereo:
                uvs = [f32(fr["matched_left_pixel_list"], 2),
                       f32(fr["matched_right_pixel_list"], 2)]
            else:
                uvs = [f32(fr["matched_pixel_list"], 2)]
            if planar:           # the single planar methods' messages
                for side, u in zip(("left_", "right_") if stereo else ("",), uvs):
                    if u.shape[0] != X.shape[0]:
                        raise RuntimeError(
                            "In PoseOnlyBundleAdjustmentSolver::"
                            "SolveMonocularPoseOnlyBundleAdjustment3Dof(), "
                            "world_position_list.size() != %scurrent_pixel_list.size()"
                            % side)
            elif any(u.shape[0] != X.shape[0] for u in uvs):
                tag = ("SolveStereoPoseOnlyBundleAdjustment6Dof" if stereo else
                       "SolveMonocularPoseOnlyBundleAdjustment6Dof")
                raise RuntimeError(
                    "In PoseOnlyBundleAdjustmentSolver::%s(), "
                    "world_position_list.size() != current_pixel_list.size()" % tag)
            prep.append((X, uvs))
        self.debug_poses_ = []
        mkeys = (("mask_inlier_left", "mask_l"), ("mask_inlier_right", "mask_r")) \
            if stereo else (("mask_inlier", "mask"),)
        if planar:
            pkey = "world_to_current_pose" if stereo else "pose_world_to_current"
        else:
            pkey = "reference_to_current_left_pose" if stereo else "reference_to_current_pose"
        live = []
        for k, (fr, (X, uvs)) in enumerate(zip(frames, prep)):
            self._begin_summary(options, fr.get("summary"))
            if X.shape[0] == 0:     # nothing to solve: masks resized, pose kept
                for mk, _ in mkeys:
                    self._write_mask(fr[mk], np.zeros(0, bool))
            else:
                live.append(k)
        ok = [True] * len(frames)
        if not live:
            return ok
        ns = [prep[k][0].shape[0] for k in live]
        off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
        cat = lambda j: np.concatenate([prep[k][1][j] for k in live])
        X = np.concatenate([prep[k][0] for k in live])
        T = np.stack([to12(frames[k][pkey]) for k in live])
        poses = lambda key: np.stack([to12(frames[k][key]) for k in live])
        masks = [np.concatenate([self._fit_mask(frames[k][mk], prep[k][0].shape[0])
                                 for k in live]) for mk, _ in mkeys]
        if stereo:
            il = [[frames[k]["fx_left"], frames[k]["fy_left"], frames[k]["cx_left"],
                   frames[k]["cy_left"]] for k in live]
            ir = [[frames[k]["fx_right"], frames[k]["fy_right"], frames[k]["cx_right"],
                   frames[k]["cy_right"]] for k in live]
            Tlr = poses("left_to_right_pose")
            if planar:
                res = self._p.pose_only_stereo3_batch(
                    off, X, cat(0), cat(1), il, ir, poses("base_to_camera_pose"), Tlr,
                    poses("world_to_last_pose"), T, masks[0], masks[1], options.to_c())
            else:
                res = self._p.pose_only_stereo6_batch(off, X, cat(0), cat(1), il, ir, Tlr, T,
                                                      masks[0], masks[1], options.to_c())
        else:
            intr = [[frames[k]["fx"], frames[k]["fy"], frames[k]["cx"], frames[k]["cy"]]
                    for k in live]
            if planar:
                res = self._p.pose_only_mono3_batch(
                    off, X, cat(0), intr, poses("pose_base_to_camera"),
                    poses("pose_world_to_last"), T, masks[0], options.to_c())
            else:
                res = self._p.pose_only_mono6_batch(off, X, cat(0), intr, T, masks[0],
                                                    options.to_c())
        for k, r in zip(live, res):
            fr = frames[k]
            r["debug"] = []
            ok[k] = self._finish_pose_only(r, fr[pkey], [(fr[mk], rk) for mk, rk in mkeys],
                                           fr.get("summary"), t0)
        self.debug_poses_ = []
        return ok

    @staticmethod
    def _write_mask(mask, values):
        if isinstance(mask, list):
            mask[:] = [bool(v) for v in values]
        else:
            mask[...] = values

    def Solve_Monocular_6Dof_Batch(self, frames, options):
        """Many Solve_Monocular_6Dof problems in one GPU launch
        (ba_pose_only_mono6_batch).  `frames` is a list of dicts keyed by
        Solve_Monocular_6Dof's parameter names (reference_position_list,
        matched_pixel_list, fx, fy, cx, cy, reference_to_current_pose,
        mask_inlier, and optionally summary); poses, masks and summaries are
        updated in place as that method updates them, and every frame gets
        the bits the single call would give it (frames of <= 2048 points).
        Returns the per-frame success flags.  A frame without points is left
        as is (mask emptied, success).  GetDebugPoses() is empty afterwards."""
        return self._solve_batch(frames, options, False)

    def Solve_Stereo_6Dof_Batch(self, frames, options):
        """Many Solve_Stereo_6Dof problems in one GPU launch
        (ba_pose_only_stereo6_batch); frames are dicts keyed by that method's
        parameter names (reference_position_list, matched_left_pixel_list,
        matched_right_pixel_list, fx_left .. cy_right, left_to_right_pose,
        reference_to_current_left_pose, mask_inlier_left, mask_inlier_right,
        and optionally summary).  As Solve_Monocular_6Dof_Batch."""
        return self._solve_batch(frames, options, True)

    def Solve_Monocular_Planar3Dof_Batch(self, frames, options):
        """Many Solve_Monocular_Planar3Dof problems in one GPU launch
        (ba_pose_only_mono3_batch).  `frames` is a list of dicts keyed by
        Solve_Monocular_Planar3Dof's parameter names (world_position_list,
        matched_pixel_list, fx, fy, cx, cy, pose_base_to_camera,
        pose_world_to_last, pose_world_to_current, mask_inlier, and optionally
        summary); poses, masks and summaries are updated in place as that
        method updates them, and every frame gets the bits the single call
        would give it (frames of <= 2048 points).  Returns the per-frame
        success flags.  Every size check comes before any device use.  A frame
        without points is left as is (mask emptied, success), where the single
        planar call rejects n = 0 instead.  GetDebugPoses() is empty
        afterwards."""
        return self._solve_batch(frames, options, False, planar=True)

    def Solve_Stereo_Planar3Dof_Batch(self, frames, options):
        """Many Solve_Stereo_Planar3Dof problems in one GPU launch
        (ba_pose_only_stereo3_batch); frames are dicts keyed by that method's
        parameter names (world_position_list, matched_left_pixel_list,
        matched_right_pixel_list, fx_left .. cy_right, base_to_camera_pose,
        left_to_right_pose, world_to_last_pose, world_to_current_pose,
        mask_inlier_left, mask_inlier_right, and optionally summary).  As
        Solve_Monocular_Planar3Dof_Batch."""
        return self._solve_batch(frames, options, True, planar=True)

    def Solve_Monocular_Planar3Dof(self, world_position_list,
                                   matched_pixel_list, fx, fy, cx, cy,
                                   pose_base_to_camera, pose_world_to_last,
                                   pose_world_to_current, mask_inlier,
                                   options, summary=None):
        """reference core/pose_only_bundle_adjustment_solver.cpp:401-615.
        Poses are 4x4 arrays; `pose_world_to_current` is updated in place
        (with pose_b2b1^-1 * pose_base_to_camera, :549-551), `mask_inlier` a
        list/array resized to n (True) and updated in place.  The positions
        are base-1 coordinates (the reference does not warp them)."""
        t0 = time.perf_counter()
        self._begin_summary(options, summary)
        self.debug_poses_ = []
        X = np.asarray(world_position_list, np.float32).reshape(-1, 3)
        uv = np.asarray(matched_pixel_list, np.float32).reshape(-1, 2)
        if X.shape[0] != uv.shape[0]:
            raise RuntimeError(
                "In PoseOnlyBundleAdjustmentSolver::"
                "SolveMonocularPoseOnlyBundleAdjustment3Dof(), "
                "world_position_list.size() != current_pixel_list.size()")
        n = X.shape[0]
        to12 = lambda T: _T44_to_12(np.asarray(T, np.float64)).astype(np.float32)
        res = self._p.pose_only_mono3(
            X, uv, fx, fy, cx, cy, to12(pose_base_to_camera),
            to12(pose_world_to_last), to12(pose_world_to_current),
            self._fit_mask(mask_inlier, n), options.to_c(), want_debug=True)
        return self._finish_pose_only(res, pose_world_to_current,
                                      ((mask_inlier, "mask"),), summary, t0)

    def Solve_Stereo_Planar3Dof(self, world_position_list,
                                matched_left_pixel_list,
                                matched_right_pixel_list, fx_left, fy_left,
                                cx_left, cy_left, fx_right, fy_right,
                                cx_right, cy_right, base_to_camera_pose,
                                left_to_right_pose, world_to_last_pose,
                                world_to_current_pose, mask_inlier_left,
                                mask_inlier_right, options, summary=None):
        """reference core/pose_only_bundle_adjustment_solver.cpp:617-900.
        As Solve_Monocular_Planar3Dof, plus the right camera at
        left_to_right_pose^-1 * left; a right pixel with a negative coordinate
        means "not matched in the right image"."""
        t0 = time.perf_counter()
        self._begin_summary(options, summary)
        self.debug_poses_ = []
        X = np.asarray(world_position_list, np.float32).reshape(-1, 3)
        ul = np.asarray(matched_left_pixel_list, np.float32).reshape(-1, 2)
        ur = np.asarray(matched_right_pixel_list, np.float32).reshape(-1, 2)
        for side, u in (("left", ul), ("right", ur)):
            if X.shape[0] != u.shape[0]:
                raise RuntimeError(
                    "In PoseOnlyBundleAdjustmentSolver::"
                    "SolveMonocularPoseOnlyBundleAdjustment3Dof(), "
                    "world_position_list.size() != %s_current_pixel_list.size()"
                    % side)
        n = X.shape[0]
        to12 = lambda T: _T44_to_12(np.asarray(T, np.float64)).astype(np.float32)
        res = self._p.pose_only_stereo3(
            X, ul, ur, [fx_left, fy_left, cx_left, cy_left],
            [fx_right, fy_right, cx_right, cy_right], to12(base_to_camera_pose),
            to12(left_to_right_pose), to12(world_to_last_pose),
            to12(world_to_current_pose), self._fit_mask(mask_inlier_left, n),
            self._fit_mask(mask_inlier_right, n), options.to_c(),
            want_debug=True)
        return self._finish_pose_only(
            res, world_to_current_pose,
            ((mask_inlier_left, "mask_l"), (mask_inlier_right, "mask_r")),
            summary, t0)


class FullBundleAdjustmentSolverRefactor(FullBundleAdjustmentSolver):
    """Mirror of reference core/full_bundle_adjustment_solver_refactor.h:
    117-136: the same device path behind the refactored names, plus the
    solver_type switch of its Solve (reference ..._refactor.cpp:944-982):
    LEVENBERG_MARQUARDT, or GAUSS_NEWTON = every step accepted with lambda fixed
    at initial_lambda (the default of Options); and
    SolveByGradientDescent (reference ..._refactor.cpp:1075-1367)."""

    def RegisterCamera(self, camera_id, camera):
        return self.AddCamera(camera_id, camera)

    def RegisterWorldToBodyPose(self, original_pose):
        return self.AddPose(original_pose)

    def RegisterWorldPoint(self, original_point):
        return self.AddPoint(original_point)

    def _use_gauss_newton(self, options):
        if options.solver_type == SolverType.LEVENBERG_MARQUARDT:
            return False
        if options.solver_type == SolverType.GAUSS_NEWTON:
            return True
        raise RuntimeError("FullBundleAdjustmentSolverRefactor::Solve: "
                           "solver_type must be GAUSS_NEWTON or "
                           "LEVENBERG_MARQUARDT")

    def SolveByGradientDescent(self, options, summary=None):
        """reference ..._refactor.cpp:1075-1367: first-order steps, each
        pose / point block clipped to norm 1e-3 (scaled units), every step
        taken; rows as documented at ba_solve_gd (include/ba_hip.h).
        solver_type, decrease / increase_ratio_lambda are ignored."""
        t0 = time.perf_counter()
        _begin_summary(summary, options)
        self.FinalizeParameters()
        if self.verbose:
            self.GetSolverStatistics()
        self.CheckPoseAndPointConnectivity()            # reference :1161
        rows, converged = self._problem.solve_gd(options.to_c())
        return self._finish_solve(rows, converged, summary, t0)
