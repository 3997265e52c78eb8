"""Host reference of the Sim(3) pose graph (ba_sim3_*): the definition of
include/ba_hip.h restated in numpy fp64.  Exponential and logarithm are scipy.linalg.expm /
logm of the 4x4 matrix [[sR, t], [0, 1]]: no closed form, nothing shared with the library.

A similarity is 13 doubles {R row-major, t, s}; a graph is a dict: pose_S (n, 13), pose_fixed
(n,), rels = dict(j, k, Z (F, 13), Omega (F, 7, 7)).

chi2:          sum_f r_f^T Omega_f r_f
dense_system:  H (7N, 7N) and g (7N) over the optimisable poses in the user's order
lm:            the chi-square LM of pgo_ref.lm at width 7 -> (rows, converged, poses)
"""
import types

import numpy as np
import scipy.linalg


def mat(S):
    """S13 -> the 4x4 matrix [[sR, t], [0, 1]]"""
    S = np.asarray(S, np.float64).reshape(13)
    M = np.eye(4)
    M[:3, :3] = S[12] * S[:9].reshape(3, 3)
    M[:3, 3] = S[9:12]
    return M


def from_mat(M):
    """the 4x4 matrix -> S13; s = det(sR)^(1/3), R the rotation nearest to sR / s (polar factor by
    an SVD).  A product of a few 4x4 matrices leaves sR / s orthogonal to some 1e-15 only; a pose
    is (R, t, s) with R a rotation, and with |s t| of 1e3 the transpose and the matrix inverse of
    an R that far off differ by 1e-12 in t_E = t_j - (s_j / s_k) R_E t_k.  Projecting here keeps
    every pose the reference hands out a rotation to rounding, so that this ambiguity stays at
    the rounding of either side."""
    A = np.asarray(M, np.float64)[:3, :3]
    s = np.cbrt(np.linalg.det(A))
    U, _, Vt = np.linalg.svd(A / s)
    return np.r_[(U @ Vt).reshape(9), M[:3, 3], s]


def hat(xi):
    """the algebra element [[hat(omega) + sigma I, v], [0, 0]] of xi = [v; omega; sigma]"""
    v, w, sg = xi[:3], xi[3:6], xi[6]
    X = np.zeros((4, 4))
    X[:3, :3] = np.array([[sg, -w[2], w[1]], [w[2], sg, -w[0]], [-w[1], w[0], sg]])
    X[:3, 3] = v
    return X


def vee(X):
    X = np.real(np.asarray(X))
    A = X[:3, :3]
    return np.r_[X[:3, 3], 0.5 * (A[2, 1] - A[1, 2]), 0.5 * (A[0, 2] - A[2, 0]), 0.5 * (A[1, 0] - A[0, 1]),
                 np.trace(A) / 3.0]


def exp_mat(xi):
    return scipy.linalg.expm(hat(np.asarray(xi, np.float64)))


def exp(xi):
    return from_mat(exp_mat(xi))


def log_mat(M):
    return vee(scipy.linalg.logm(np.asarray(M, np.float64)))


def log(S):
    return log_mat(mat(S))


def compose(Sa, Sb):
    return from_mat(mat(Sa) @ mat(Sb))


def inverse(S):
    return from_mat(np.linalg.inv(mat(S)))


def E_of(Sj, Sk):
    return mat(Sj) @ np.linalg.inv(mat(Sk))


def residual(Sj, Sk, Z):
    return log_mat(E_of(Sj, Sk) @ np.linalg.inv(mat(Z)))


def adjoint(S):
    """Ad7 of the definition: [[sR, hat(t) R, -t], [0, R, 0], [0, 0, 1]]"""
    S = np.asarray(S, np.float64).reshape(13)
    R, t, s = S[:9].reshape(3, 3), S[9:12], S[12]
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ad = np.zeros((7, 7))
    Ad[:3, :3] = s * R
    Ad[:3, 3:6] = tx @ R
    Ad[:3, 6] = -t
    Ad[3:6, 3:6] = R
    Ad[6, 6] = 1.0
    return Ad


def sym_lower(O):
    O = np.asarray(O, np.float64).reshape(7, 7)
    L = np.tril(O)
    return L + np.tril(O, -1).T


def n_factors(rels):
    return len(np.asarray(rels["j"]).reshape(-1))


def chi2_terms(S, rels):
    S = np.asarray(S, np.float64).reshape(-1, 13)
    out = np.zeros(n_factors(rels))
    for f in range(len(out)):
        r = residual(S[int(rels["j"][f])], S[int(rels["k"][f])], rels["Z"][f])
        out[f] = r @ sym_lower(rels["Omega"][f]) @ r
    return out


def chi2(S, rels):
    out = 0.0
    for v in chi2_terms(S, rels):
        out += v
    return out


def dense_system(pose_fixed, S, rels):
    """H_jj += Omega, H_kk += Ad^T Omega Ad, H_jk += -Omega Ad, g_j += -Omega r, g_k += Ad^T Omega r"""
    S = np.asarray(S, np.float64).reshape(-1, 13)
    fixed = np.asarray(pose_fixed).reshape(-1)
    opt = np.full(len(fixed), -1)
    opt[fixed == 0] = np.arange(int((fixed == 0).sum()))
    N = int((fixed == 0).sum())
    H, g = np.zeros((7 * N, 7 * N)), np.zeros(7 * N)
    for f in range(n_factors(rels)):
        j, k = int(rels["j"][f]), int(rels["k"][f])
        E = from_mat(E_of(S[j], S[k]))
        r = residual(S[j], S[k], rels["Z"][f])
        Om, Ad = sym_lower(rels["Omega"][f]), adjoint(E)
        a, b = opt[j], opt[k]
        if a >= 0:
            H[7 * a:7 * a + 7, 7 * a:7 * a + 7] += Om
            g[7 * a:7 * a + 7] -= Om @ r
        if b >= 0:
            H[7 * b:7 * b + 7, 7 * b:7 * b + 7] += Ad.T @ Om @ Ad
            g[7 * b:7 * b + 7] += Ad.T @ (Om @ r)
        if a >= 0 and b >= 0:
            H[7 * a:7 * a + 7, 7 * b:7 * b + 7] -= Om @ Ad
            H[7 * b:7 * b + 7, 7 * a:7 * a + 7] -= (Om @ Ad).T
    return H, g


def solve_numpy(A, b):
    return np.linalg.solve(A, b)


def solve_cholesky(A, b):
    return scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), b)


def moved(S, x, opt):
    """S_j <- sim3_exp(x_j) S_j on the optimisable poses `opt`"""
    out = np.array(S, np.float64)
    for n, p in enumerate(opt):
        out[p] = from_mat(exp_mat(x[7 * n:7 * n + 7]) @ mat(out[p]))
    return out


def lm(graph, opt, solve=solve_numpy):
    """-> (rows, converged, poses (n, 13)): pgo_ref.lm at width 7"""
    fixed = np.asarray(graph["pose_fixed"])
    rels = graph["rels"]
    S = np.array(graph["pose_S"], np.float64).reshape(-1, 13)
    ps = np.flatnonzero(fixed == 0)
    F = n_factors(rels)
    lam = float(opt.initial_lambda)
    acc = chi2(S, rels)
    rows, conv = [], False
    for it in range(opt.max_num_iterations):
        H, g = dense_system(fixed, S, rels)
        d = np.diag(H).copy()
        x = solve(H + lam * np.diag(d), g)
        St = moved(S, x, ps)
        trial = chi2(St, rels)
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
        step = np.linalg.norm(x.reshape(-1, 7), axis=1).sum() / len(ps)
        conv = bool(step < float(opt.threshold_step_size) or change < float(opt.threshold_cost_change))
        if it >= opt.max_num_iterations - 1:
            conv = False
        if accept:
            S, acc = St, trial
        rows.append(types.SimpleNamespace(
            iteration_status=status, damping_term=lam, trial_cost=trial, rho=rho, model_change=pred,
            abs_step=step, cost=acc, cost_change=change if accept else 0.0,
            average_reprojection_error=np.sqrt(acc / F)))
        if conv:
            break
    return rows, conv, S


def pose_distance(Sa, Sb):
    """max_j |sim3_log(Sa_j Sb_j^-1)|"""
    out = 0.0
    for a, b in zip(np.asarray(Sa).reshape(-1, 13), np.asarray(Sb).reshape(-1, 13)):
        out = max(out, np.linalg.norm(log_mat(E_of(a, b))))
    return out
