"""Host reference of the robust Sim(3) pose graph (ba_sim3_set_robust): chi2,
dense_system and lm of sim3_ref.py restated with a kernel kind and a scale c per factor.  A graph
is the dict of sim3_ref with two more keys, kind (F,) and scale (F,).  The unweighted pieces
(residual, adjoint, exp / log by scipy expm / logm) are sim3_ref's; nothing is shared with the
library.

rho, weight:   the table of include/ba_hip.h, elementwise
factor_s:      s_f = r_f^T Omega_f r_f, r of 7 components
cost:          sum_f rho_f(s_f)
system:        sim3_ref.dense_system with w_f Omega_f for Omega_f, w_f at the poses given
lm:            sim3_ref.lm with cost for chi-square and system for the dense system; w_f at the
               accepted poses -> (rows, converged, poses).  trace: a list that receives s of every
               factor at every accepted and trial pose the loop visits
"""
import types

import numpy as np

import sim3_ref
from sim3_ref import moved, solve_cholesky, solve_numpy  # noqa: F401  (the two solves of the noise rule)

NONE, HUBER, CAUCHY, GM = 0, 1, 2, 3


def rho(kind, c, s):
    kind, c, s = np.broadcast_arrays(np.asarray(kind), np.asarray(c, np.float64), np.asarray(s, np.float64))
    c2 = c * c
    out = np.array(s, np.float64)
    with np.errstate(all="ignore"):
        h = (kind == HUBER) & (s > c2)
        out[h] = (2.0 * c * np.sqrt(s) - c2)[h]
        m = kind == CAUCHY
        out[m] = (c2 * np.log1p(s / c2))[m]
        m = kind == GM
        out[m] = (c2 / (c2 + s) * s)[m]
    return out


def weight(kind, c, s):
    kind, c, s = np.broadcast_arrays(np.asarray(kind), np.asarray(c, np.float64), np.asarray(s, np.float64))
    c2 = c * c
    out = np.ones(s.shape)
    with np.errstate(all="ignore"):
        h = (kind == HUBER) & (s > c2)
        out[h] = (c / np.sqrt(s))[h]
        m = kind == CAUCHY
        out[m] = (1.0 / (1.0 + s / c2))[m]
        m = kind == GM
        out[m] = ((c2 / (c2 + s)) ** 2)[m]
    return out


def factor_s(S, rels):
    return sim3_ref.chi2_terms(S, rels)


def kernels(graph):
    F = sim3_ref.n_factors(graph["rels"])
    kind = np.asarray(graph.get("kind", np.zeros(F)), np.int32)
    scale = np.asarray(graph.get("scale", np.ones(F)), np.float64)
    return kind, np.where(kind == 0, 1.0, scale)


def cost(S, graph, trace=None):
    kind, scale = kernels(graph)
    s = factor_s(S, graph["rels"])
    if trace is not None:
        trace.append(s)
    out = 0.0
    for v in rho(kind, scale, s):
        out += v
    return out


def report(S, graph):
    """-> (s, w) per factor at the poses S"""
    kind, scale = kernels(graph)
    s = factor_s(S, graph["rels"])
    return s, weight(kind, scale, s)


def system(graph, S):
    """-> (H, g): sim3_ref.dense_system with w_f Omega_f (lower triangles mirrored first)"""
    rels = graph["rels"]
    _, w = report(S, graph)
    Om = np.array([sim3_ref.sym_lower(o) for o in np.asarray(rels["Omega"]).reshape(-1, 7, 7)]) * w[:, None, None]
    return sim3_ref.dense_system(graph["pose_fixed"], S, dict(rels, Omega=Om))


def lm(graph, opt, solve=solve_numpy, trace=None):
    """-> (rows, converged, poses (n, 13))"""
    S = np.array(graph["pose_S"], np.float64).reshape(-1, 13)
    ps = np.flatnonzero(np.asarray(graph["pose_fixed"]) == 0)
    F = sim3_ref.n_factors(graph["rels"])
    lam = float(opt.initial_lambda)
    acc = cost(S, graph, trace)
    rows, conv = [], False
    for it in range(opt.max_num_iterations):
        H, g = system(graph, S)
        d = np.diag(H).copy()
        x = solve(H + lam * np.diag(d), g)
        St = moved(S, x, ps)
        trial = cost(St, graph, trace)
        if opt.gauss_newton:
            status, gain, pred, accept = 0, 0.0, 0.0, True
        else:
            pred = g @ x + lam * ((x * d) @ x)
            with np.errstate(all="ignore"):
                gain = (acc - trial) / pred
            accept = bool(gain > 0.25)
            status = 0 if accept else 2
            if gain > 0.5:
                lam = max(1e-10, lam * float(opt.decrease_ratio_lambda))
                status = 1
            elif not accept:
                lam = min(1e10, lam * float(opt.increase_ratio_lambda))
        change = abs(acc - trial)
        step = np.linalg.norm(x.reshape(-1, 7), axis=1).sum() / len(ps)
        conv = bool(step < float(opt.threshold_step_size) or change < float(opt.threshold_cost_change))
        if it >= opt.max_num_iterations - 1:
            conv = False
        if accept:
            S, acc = St, trial
        rows.append(types.SimpleNamespace(
            iteration_status=status, damping_term=lam, trial_cost=trial, rho=gain, model_change=pred,
            abs_step=step, cost=acc, cost_change=change if accept else 0.0,
            average_reprojection_error=np.sqrt(acc / F)))
        if conv:
            break
    return rows, conv, S
