"""CPU tests of the gradient-descent restatement (tests/gd_ref.py) and of the
ABI surface of the GPU loop (ba_gd_*): the restatement's gradient is the
derivative of the cost it models, clipping and the stop rule behave as in
reference core/full_bundle_adjustment_solver_refactor.cpp:1269-1311, and the
library exports and binds the new entry points."""
import numpy as np
import pytest

import gd_ref as G
from bundle_adjustment_solver_amd import _lib, scenes


def small_problem(seed=5):
    sc = scenes.synthetic_ba_scene(10, 120, 5, True, seed=seed, pose_noise=0.002,
                                   point_noise=0.002)
    return scenes.scaled_problem(sc)


def test_gradient_is_minus_the_derivative_of_half_the_squared_residuals():
    """Below the Huber threshold (w = 1): -a_j and -b_i are the central finite
    differences of 1/2 sum ||r||^2 under T_jw <- exp(d) T_jw and X_i <- X_i + d."""
    pr = small_problem()
    P = G.Problem(pr)
    R, t = G.split12(pr["pose_T"])
    X = pr["pt_X"].reshape(-1, 3).copy()
    r = G.project(P, R, t, X)[0]
    assert (np.abs(r).sum(1) < 1e3).all()
    a, b = G.gradient(P, R, t, X, huber=1e3)   # no observation above the threshold

    def half_sq(R_, t_, X_):
        rr = G.project(P, R_, t_, X_)[0]
        return 0.5 * float((rr ** 2).sum())

    h = 1e-6
    for jo in (0, len(P.opt_poses) // 2, len(P.opt_poses) - 1):
        j = P.opt_poses[jo]
        fd = np.zeros(6)
        for k in range(6):
            f = []
            for s in (1, -1):
                d = np.zeros(6)
                d[k] = s * h
                dR, dt = G.se3_exp(d)
                R2, t2 = R.copy(), t.copy()
                R2[j], t2[j] = dR[0] @ R[j], dR[0] @ t[j] + dt[0]
                f.append(half_sq(R2, t2, X))
            fd[k] = (f[0] - f[1]) / (2 * h)
        assert np.abs(-a[jo] - fd).max() <= 1e-6 * np.abs(fd).max()
    for io in (0, len(P.opt_points) // 2, len(P.opt_points) - 1):
        i = P.opt_points[io]
        fd = np.zeros(3)
        for k in range(3):
            f = []
            for s in (1, -1):
                X2 = X.copy()
                X2[i, k] += s * h
                f.append(half_sq(R, t, X2))
            fd[k] = (f[0] - f[1]) / (2 * h)
        assert np.abs(-b[io] - fd).max() <= 1e-6 * np.abs(fd).max()


def test_huber_weight_applied_once():
    pr = small_problem()
    P = G.Problem(pr)
    R, t = G.split12(pr["pose_T"])
    X = pr["pt_X"].reshape(-1, 3)
    r = G.project(P, R, t, X)[0]
    huber = float(np.median(np.abs(r).sum(1)))
    a1, b1 = G.gradient(P, R, t, X, huber)
    a0, b0 = G.gradient(P, R, t, X, 1e30)
    assert not np.allclose(b1, b0)
    # w r = huber r / (|rx| + |ry|): an observation above the threshold contributes
    # with a residual of L1 norm exactly `huber`
    absr = np.abs(r).sum(1)
    P2 = G.Problem(dict(pr, obs_uv=pr["obs_uv"]))
    scale = np.where(absr > huber, huber / absr, 1.0)
    P2.uv = P.uv + (r - scale[:, None] * r)       # residuals scaled by the weight
    a2, b2 = G.gradient(P2, R, t, X, 1e30)
    assert np.allclose(a1, a2, rtol=1e-6, atol=1e-9 * np.abs(a1).max())
    assert np.allclose(b1, b2, rtol=1e-6, atol=1e-9 * np.abs(b1).max())


def test_clip_bounds_the_norm_and_keeps_the_direction():
    rng = np.random.default_rng(3)
    for dim in (3, 6):
        v = rng.normal(size=(500, dim)) * rng.choice([1e-5, 1e-3, 1.0, 1e3], size=(500, 1))
        c = G.clip(v)
        n0, n1 = np.linalg.norm(v, axis=1), np.linalg.norm(c, axis=1)
        assert (n1 <= G.MAX_STEP * (1 + 1e-15)).all()
        small = n0 <= G.MAX_STEP
        assert (c[small] == v[small]).all()
        cos = (v * c).sum(1) / (n0 * n1)
        assert np.allclose(cos[~small], 1.0, atol=1e-14)
        assert np.allclose(n1[~small], G.MAX_STEP, rtol=1e-14)


def test_stop_rule_and_last_iteration_override():
    conv, m = G.stop_rule(0.5, 10.0, 1.0, 1e-5, iteration=0, max_iteration=10)
    assert conv and m == pytest.approx(0.5)             # step rule
    conv, _ = G.stop_rule(2.0, 1e-6, 1.0, 1e-5, 3, 10)
    assert conv                                          # cost-change rule
    conv, m = G.stop_rule(2.0, 1.0, 1.0, 1e-5, 3, 10)
    assert not conv and m == pytest.approx(1.0)
    conv, _ = G.stop_rule(0.5, 1e-6, 1.0, 1e-5, 9, 10)  # last allowed iteration
    assert not conv


def test_solve_quirks_and_zero_iterations():
    pr = small_problem(seed=6)
    out = G.solve(pr, max_iter=0)
    assert out["rows"] == [] and not out["converged"]
    assert (out["T_jw12"] == pr["pose_T"]).all() and (out["X"] == pr["pt_X"]).all()
    out = G.solve(pr, max_iter=6, thr_step=0.0, thr_cost=0.0, initial_lambda=1e-3)
    rows = out["rows"]
    assert len(rows) == 6 and not out["converged"]
    n_obs = len(pr["obs_uv"])
    prev = out["initial_cost"]
    N, M = int((pr["pose_fixed"] == 0).sum()), int((pr["pt_fixed"] == 0).sum())
    for r, (a, b) in zip(rows, out["grads"]):
        assert r["average_reprojection_error"] == r["cost"] / n_obs     # no sqrt
        assert r["cost_change"] == abs(r["cost"] - prev)
        step = ((0.01 + np.linalg.norm(G.clip(b), axis=1).sum())
                + (0.01 + np.linalg.norm(G.clip(a), axis=1).sum())) / (N + M)
        assert r["abs_step"] == pytest.approx(step, rel=1e-15)
        assert r["damping_term"] == float(np.float32(1e-3)) and r["abs_gradient"] == 0.0
        assert r["iteration_status"] == 0
        prev = r["cost"]
    # a step threshold above the step measure stops at once; not on the last iteration
    big = G.solve(pr, max_iter=5, thr_step=1.0, thr_cost=0.0)
    assert len(big["rows"]) == 1 and big["converged"]
    last = G.solve(pr, max_iter=1, thr_step=1.0, thr_cost=0.0)
    assert len(last["rows"]) == 1 and not last["converged"]
    # fixed poses and points do not move
    fixed = np.nonzero(pr["pose_fixed"])[0]
    assert (out["T_jw12"][fixed] == pr["pose_T"][fixed]).all()


def test_library_exports_and_binds_gradient_descent(built):
    lib = _lib.load()
    for name in ("ba_solve_gd", "ba_gd_begin", "ba_gd_iterate", "ba_gd_sync",
                 "ba_gd_get_gradient"):
        assert hasattr(lib, name), "missing export: " + name
        assert name in _lib.SIGNATURES, "no ctypes signature for " + name
    from bundle_adjustment_solver_amd.solver import BaProblem
    for m in ("solve_gd", "gd_begin", "gd_iterate", "gd_sync", "gd_gradient"):
        assert callable(getattr(BaProblem, m))
