"""Host reference of the pose-graph optimisation (ba_pgraph_*): the definition
of include/ba_hip.h in numpy fp64 with a dense solve.  The arithmetic is the project's existing
host statement: rel_ref.dense_factors for H and g, solver.relative_residual for r.

A graph is a dict: pose_T (n, 12) T_jw in scaled units, pose_fixed (n,), rels the dict of
rel_ref (j, k, Z, Omega).

chi2:            sum_f r_f^T Omega_f r_f
lm:              the chi-square LM of the definition -> (rows, converged, poses)
lm_full_control: the full solver's control (rel_ref.lm_with_relatives) restated without the
                 observation terms: sum of norms against the quadratic model times 100, the
                 trial cost kept as "previous" after a rejection
"""
import types

import numpy as np
import scipy.linalg

from bundle_adjustment_solver_amd.solver import relative_residual, se3_log

import rel_ref
from prior_ref import compose, se3_exp, sym_lower


def chi2(T, rels):
    out = 0.0
    for f in range(rel_ref.n_factors(rels)):
        r = relative_residual(T[int(rels["j"][f])], T[int(rels["k"][f])], rels["Z"][f])
        out += r @ sym_lower(rels["Omega"][f]) @ r
    return out


def solve_numpy(A, b):
    return np.linalg.solve(A, b)


def solve_cholesky(A, b):
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), b)


def moved(T, x, opt):
    """T_j <- se3_exp(x_j) T_j on the optimisable poses `opt`"""
    out = np.array(T, np.float64)
    for n, p in enumerate(opt):
        out[p] = compose(se3_exp(x[6 * n:6 * n + 6]), out[p])
    return out


def lm(graph, opt, solve=solve_numpy):
    """-> (rows, converged, poses (n, 12))"""
    pr = dict(pose_fixed=np.asarray(graph["pose_fixed"]))
    rels = graph["rels"]
    T = np.array(graph["pose_T"], np.float64).reshape(-1, 12)
    ps = np.flatnonzero(pr["pose_fixed"] == 0)
    F = rel_ref.n_factors(rels)
    lam = float(opt.initial_lambda)
    acc = chi2(T, rels)
    rows, conv = [], False
    for it in range(opt.max_num_iterations):
        H, g = rel_ref.dense_factors(pr, T, rels)
        d = np.diag(H).copy()
        x = solve(H + lam * np.diag(d), g)
        Tt = moved(T, x, ps)
        trial = chi2(Tt, rels)
        if opt.gauss_newton:
            status, rho, pred, accept = 0, 0.0, 0.0, True
        else:
            pred = g @ x + lam * ((x * d) @ x)
            with np.errstate(all="ignore"):
                rho = (acc - trial) / pred
            accept = bool(rho > 0.25)
            status = 0 if accept else 2
            if rho > 0.5:
                lam = max(1e-10, lam * float(opt.decrease_ratio_lambda))
                status = 1
            elif not accept:
                lam = min(1e10, lam * float(opt.increase_ratio_lambda))
        change = abs(acc - trial)
        step = np.linalg.norm(x.reshape(-1, 6), axis=1).sum() / len(ps)
        conv = bool(step < float(opt.threshold_step_size) or change < float(opt.threshold_cost_change))
        if it >= opt.max_num_iterations - 1:
            conv = False
        if accept:
            T, acc = Tt, trial
        rows.append(types.SimpleNamespace(
            iteration_status=status, damping_term=lam, trial_cost=trial, rho=rho, model_change=pred,
            abs_step=step, cost=acc, cost_change=change if accept else 0.0,
            average_reprojection_error=np.sqrt(acc / F)))
        if conv:
            break
    return rows, conv, T


def lm_full_control(graph, opt):
    """rel_ref.lm_with_relatives without the observation terms -> rows"""
    pr = dict(pose_fixed=np.asarray(graph["pose_fixed"]))
    rels = graph["rels"]
    T = np.array(graph["pose_T"], np.float64).reshape(-1, 12)
    ps = np.flatnonzero(pr["pose_fixed"] == 0)
    lam = float(opt.initial_lambda)
    prev = rel_ref.rel_norm(T, rels)
    rows = []
    for it in range(opt.max_num_iterations):
        H, g = rel_ref.dense_factors(pr, T, rels)
        Hd = H + lam * np.diag(np.diag(H))
        x = np.linalg.solve(Hd, g)
        Tt = moved(T, x, ps)
        cur = rel_ref.rel_norm(Tt, rels)
        model = -(g @ x + x @ Hd @ x)
        with np.errstate(all="ignore"):
            rho = (cur - prev) * 100.0 / model
        status = 0
        if rho > 0.25:
            T = Tt
        else:
            status = 2
        if rho > 0.5:
            lam = max(1e-10, lam * float(opt.decrease_ratio_lambda))
            status = 1
        elif rho <= 0.25:
            lam = min(100.0, lam * float(opt.increase_ratio_lambda))
        rows.append(types.SimpleNamespace(iteration_status=status, damping_term=lam, trial_cost=cur, rho=rho))
        prev = cur   # even when skipped
    return rows


def pose_distance(Ta, Tb):
    """max_j |se3_log(Ta_j Tb_j^-1)|"""
    out = 0.0
    for a, b in zip(np.asarray(Ta).reshape(-1, 12), np.asarray(Tb).reshape(-1, 12)):
        out = max(out, np.linalg.norm(se3_log(compose(a, rel_ref.inverse12(b)))))
    return out
