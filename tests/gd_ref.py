"""CPU restatement (numpy float64) of the reference's
FullBundleAdjustmentSolverRefactor::SolveByGradientDescent,
core/full_bundle_adjustment_solver_refactor.cpp:1075-1367, with the cost of
:375-427, the update of :482-503 and se3Exp of :1370-1409.

Test infrastructure only: the product path (bundle_adjustment_solver_amd/)
never imports it.  It works on the SCALED arrays of scenes.scaled_problem (the
C-ABI level: T_jw = pose^-1, 0.01 scaling).  The per-observation loop is
vectorised, so sums are accumulated in another order than the reference's
sequential loop (they differ at roundoff).  Quirks kept on purpose:
  * the cost is sum ||r|| (not squared) over EVERY observation, fixed poses and
    points included;
  * the weight w = huber / (|rx| + |ry|) above the threshold is applied once;
  * each block is clipped to norm 1e-3 on its own, every step is taken;
  * average_reprojection_error = cost / observations, without a sqrt;
  * the step measure is (0.01 + sum ||a_j|| + 0.01 + sum ||b_i||) / (N + M) of
    the CLIPPED blocks;
  * the last allowed iteration never reports convergence;
  * damping_term = initial_lambda, abs_gradient = 0, status UPDATE.
Every stop decision also carries its margin to each threshold, so that a test
can tell a real difference from one that roundoff could flip."""
import numpy as np

MAX_STEP = 0.001  # max_pose_step = max_point_step (:1272-1273)
F32 = np.float32


def split12(T12):
    T12 = np.asarray(T12, np.float64).reshape(-1, 12)
    return T12[:, :9].reshape(-1, 3, 3), T12[:, 9:]


def join12(R, t):
    return np.concatenate([R.reshape(-1, 9), t.reshape(-1, 3)], axis=1)


def hat(w):
    w = np.asarray(w, np.float64).reshape(-1, 3)
    z = np.zeros(len(w))
    return np.stack([np.stack([z, -w[:, 2], w[:, 1]], 1),
                     np.stack([w[:, 2], z, -w[:, 0]], 1),
                     np.stack([-w[:, 1], w[:, 0], z], 1)], 1)


def se3_exp(x):
    """exp of x = (v, w) rows -> (dR [n,3,3], dt [n,3]) (reference :1370-1409)."""
    x = np.asarray(x, np.float64).reshape(-1, 6)
    v, w = x[:, :3], x[:, 3:]
    th = np.linalg.norm(w, axis=1)
    W = hat(w)
    W2 = W @ W
    small = th < 1e-7
    ths = np.where(small, 1.0, th)
    ca = np.where(small, 1.0, np.sin(ths) / ths)
    cb = np.where(small, 0.5, (1.0 - np.cos(ths)) / ths ** 2)
    vb = np.where(small, 1.0 / 3.0, (ths - np.sin(ths)) / ths ** 3)
    eye = np.eye(3)[None]
    dR = eye + ca[:, None, None] * W + cb[:, None, None] * W2
    V = eye + cb[:, None, None] * W + vb[:, None, None] * W2
    return dR, np.einsum("nij,nj->ni", V, v)


class Problem:
    """The scaled problem (dict of scenes.scaled_problem) with its index maps:
    opt poses / points are the non-fixed ones in input order."""

    def __init__(self, pr):
        self.intr = np.asarray(pr["cam_intr"], np.float64).reshape(-1, 4)
        self.Rc, self.tc = split12(pr["cam_T"])
        self.pose_fixed = np.asarray(pr["pose_fixed"], bool)
        self.pt_fixed = np.asarray(pr["pt_fixed"], bool)
        self.cam = np.asarray(pr["obs_cam"], np.int64)
        self.pose = np.asarray(pr["obs_pose"], np.int64)
        self.pt = np.asarray(pr["obs_pt"], np.int64)
        self.uv = np.asarray(pr["obs_uv"], np.float64).reshape(-1, 2)
        self.opt_poses = np.nonzero(~self.pose_fixed)[0]
        self.opt_points = np.nonzero(~self.pt_fixed)[0]
        self.jopt = np.full(len(self.pose_fixed), -1)
        self.jopt[self.opt_poses] = np.arange(len(self.opt_poses))
        self.iopt = np.full(len(self.pt_fixed), -1)
        self.iopt[self.opt_points] = np.arange(len(self.opt_points))


def project(P, R, t, X):
    """Residuals and the pieces of the Jacobians of every observation at
    (R, t) = T_jw (all poses) and X (all points)."""
    Rj, tj = R[P.pose], t[P.pose]
    Xi = X[P.pt]
    Xij = np.einsum("nij,nj->ni", Rj, Xi) + tj                    # body frame
    Rc, tc = P.Rc[P.cam], P.tc[P.cam]
    Xc = np.einsum("nij,nj->ni", Rc, Xij) + tc                    # camera frame
    fx, fy, cx, cy = (P.intr[P.cam, k] for k in range(4))
    invz = 1.0 / Xc[:, 2]
    r = np.stack([fx * Xc[:, 0] * invz + cx, fy * Xc[:, 1] * invz + cy], 1) - P.uv
    # dpij_dXi * R_cj (:1208-1229)
    G = np.stack([fx[:, None] * invz[:, None] * Rc[:, 0, :]
                  - (fx * Xc[:, 0] * invz * invz)[:, None] * Rc[:, 2, :],
                  fy[:, None] * invz[:, None] * Rc[:, 1, :]
                  - (fy * Xc[:, 1] * invz * invz)[:, None] * Rc[:, 2, :]], 1)
    return r, G, Xij, Rj


def cost(P, R, t, X):
    """EvaluateCurrentCost (:375-427): sum of ||r|| over every observation."""
    r = project(P, R, t, X)[0]
    return float(np.sum(np.sqrt(r[:, 0] ** 2 + r[:, 1] ** 2)))


def gradient(P, R, t, X, huber):
    """(a [N,6], b [M,3]) of :1161-1267 (a_j -= Q^T w r, b_i -= R^T w r)."""
    r, G, Xij, Rj = project(P, R, t, X)
    absr = np.abs(r[:, 0]) + np.abs(r[:, 1])
    w = np.where(absr > huber, huber / np.where(absr > 0, absr, 1.0), 1.0)
    wr = w[:, None] * r
    # Q = [G, G * skew], skew = [[0, Z, -Y], [-Z, 0, X], [Y, -X, 0]] (:1238-1241)
    sk = -hat(Xij)
    Q = np.concatenate([G, G @ sk], axis=2)                       # [n,2,6]
    Rm = G @ Rj                                                   # [n,2,3]
    a = np.zeros((len(P.opt_poses), 6))
    b = np.zeros((len(P.opt_points), 3))
    jo, io = P.jopt[P.pose], P.iopt[P.pt]
    mj, mi = jo >= 0, io >= 0
    np.add.at(a, jo[mj], -np.einsum("nkc,nk->nc", Q[mj], wr[mj]))
    np.add.at(b, io[mi], -np.einsum("nkc,nk->nc", Rm[mi], wr[mi]))
    return a, b


def clip(v):
    """Per block: v *= 1e-3 / ||v|| when ||v|| > 1e-3 (:1275-1282)."""
    v = np.array(v, np.float64)
    n = np.linalg.norm(v, axis=1)
    big = n > MAX_STEP
    v[big] *= (MAX_STEP / n[big])[:, None]
    return v


def update(P, R, t, X, a, b):
    """UpdateOptimizationParameters (:482-503): T_jw <- exp(a_j) T_jw,
    X_i <- X_i + b_i, on copies."""
    R, t, X = R.copy(), t.copy(), X.copy()
    dR, dt = se3_exp(a)
    j = P.opt_poses
    R[j], t[j] = dR @ R[j], np.einsum("nij,nj->ni", dR, t[j]) + dt
    X[P.opt_points] += b
    return R, t, X


def stop_rule(step, cost_change, thr_step, thr_cost, iteration, max_iteration):
    """(:1305-1311) -> (is_converged, margin): margin = the smaller relative
    distance of the two compared quantities to their thresholds."""
    conv = (step < thr_step) or (cost_change < thr_cost)
    if iteration >= max_iteration - 1:
        conv = False
    rel = lambda v, thr: abs(v - thr) / max(abs(thr), 1e-300)
    return conv, min(rel(step, thr_step), rel(cost_change, thr_cost))


def solve(pr, max_iter=50, thr_step=1e-5, thr_cost=1e-5, huber=1.0,
          initial_lambda=100.0):
    """The whole method on the scaled problem.  Options are float in the
    reference (promoted to double where used).  Returns a dict: rows (cost,
    cost_change, average_reprojection_error, abs_step, abs_gradient,
    damping_term, iteration_status, margin), converged, T_jw12, X, and the
    per-iteration unclipped gradients."""
    P = Problem(pr)
    thr_step, thr_cost, huber, lam = (float(F32(v)) for v in
                                      (thr_step, thr_cost, huber, initial_lambda))
    R, t = split12(pr["pose_T"])
    X = np.array(pr["pt_X"], np.float64).reshape(-1, 3)
    n_obs = len(P.pose)
    if n_obs < 1:
        raise RuntimeError("SolveByGradientDescent: num_observations < 1")
    N, M = len(P.opt_poses), len(P.opt_points)
    previous = cost(P, R, t, X)                                   # :1158
    rows, grads = [], []
    converged = False
    for it in range(max_iter):
        a, b = gradient(P, R, t, X, huber)
        grads.append((a, b))
        a, b = clip(a), clip(b)
        R, t, X = update(P, R, t, X, a, b)
        current = cost(P, R, t, X)
        cost_change = abs(current - previous)
        step = ((0.01 + np.linalg.norm(b, axis=1).sum())
                + (0.01 + np.linalg.norm(a, axis=1).sum())) / (N + M)
        converged, margin = stop_rule(step, cost_change, thr_step, thr_cost,
                                      it, max_iter)
        rows.append(dict(cost=current, cost_change=cost_change,
                         average_reprojection_error=current / n_obs,
                         abs_step=step, abs_gradient=0.0, damping_term=lam,
                         iteration_status=0, margin=margin))
        previous = current
        if converged:
            break
    return dict(rows=rows, converged=converged, T_jw12=join12(R, t), X=X,
                grads=grads, initial_cost=cost(P, *split12(pr["pose_T"]),
                                               np.asarray(pr["pt_X"], np.float64).reshape(-1, 3)))
