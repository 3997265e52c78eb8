"""Host reference for the pose-prior tests (numpy / scipy fp64 and the CPU oracle, no GPU).

A prior is a dict in scaled units: poses (problem-local user indices of optimisable poses,
ascending), H (6K, 6K; only the lower triangle counts), b (6K,), T_lin (K, 12), c.

lm_with_prior: the LM loop of the oracle driven stage by stage, with the prior added on the
host: H + lambda diag(H) and g = b - H delta into the reduced system between schur and
solve_reduced, the prior's residual norm into every cost, g^T x + x^T (H + lambda diag H) x
into the model.  The control step restates reference full_bundle_adjustment_solver.cpp:
928-1007 as oracle/ba_oracle.cpp does.
marg_with_prior / cov_with_prior: marg_ref.reference and the cov_ref routes with the old
prior added to the pose block of the full normal matrix (and to g) before the elimination.
reduced_window: the window that is left when the marked poses and the landmarks of L leave.
"""
import types

import numpy as np
import scipy.linalg

from bundle_adjustment_solver_amd.solver import prior_delta
from oracle import oracle_py as O

import cov_ref
import marg_ref

OBS_KEYS = marg_ref.OBS_KEYS


def sym_lower(H):
    """the symmetric matrix whose lower triangle is H's"""
    L = np.tril(np.asarray(H, np.float64))
    return L + np.tril(L, -1).T


def se3_exp(x):
    """the library's se3_exp (csrc/ba_device_fn.h) in numpy: x = [v; w] -> T12"""
    x = np.asarray(x, np.float64)
    v, w = x[:3], x[3:]
    th = np.sqrt(w @ w)
    wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-7:
        ca, cb, va, vb = 1.0, 0.5, 0.5, 1.0 / 3.0
    else:
        ca, cb = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2
        va, vb = cb, (th - np.sin(th)) / th ** 3
    R = np.eye(3) + ca * wx + cb * wx @ wx
    V = np.eye(3) + va * wx + vb * wx @ wx
    return np.r_[R.reshape(9), V @ v]


def compose(A12, B12):
    """A B of two 12-double transforms"""
    Ra, ta = A12[:9].reshape(3, 3), A12[9:]
    Rb, tb = B12[:9].reshape(3, 3), B12[9:]
    return np.r_[(Ra @ Rb).reshape(9), Ra @ tb + ta]


def opt_cols(pr, prior):
    """columns of the prior's poses among the optimisable poses of the problem"""
    jopt = np.cumsum(np.asarray(pr["pose_fixed"]) == 0) - 1
    assert (np.asarray(pr["pose_fixed"])[prior["poses"]] == 0).all()
    return (6 * jopt[np.asarray(prior["poses"])][:, None] + np.arange(6)[None, :]).reshape(-1)


def delta_of(T, prior):
    return np.concatenate([prior_delta(T[q], prior["T_lin"][t]) for t, q in enumerate(prior["poses"])])


def prior_energy(T, prior):
    """delta^T H delta - 2 b^T delta + c at the poses T (n_pose, 12)"""
    d = delta_of(T, prior)
    return d @ sym_lower(prior["H"]) @ d - 2.0 * (prior["b"] @ d) + float(prior.get("c", 0.0))


def prior_norm(T, prior):
    return np.sqrt(max(0.0, prior_energy(T, prior)))


def lm_with_prior(pr, prior, opt):
    """-> (rows, converged, poses, points): rows carry iteration_status, damping_term, cost,
    trial_cost, rho, model_change, abs_step.  prior None: the oracle's own loop, restated."""
    o = O.Oracle(pr)
    huber = float(opt.threshold_huber_loss)
    if prior is not None:
        Hs = sym_lower(prior["H"])
        cols = opt_cols(pr, prior)
        ix = np.ix_(cols, cols)
        b = np.asarray(prior["b"], np.float64)
    pn = (lambda: prior_norm(o.get_poses(), prior)) if prior is not None else (lambda: 0.0)
    prev = o.cost() + pn() if prior is not None else o.cost()
    lam = float(opt.initial_lambda)
    rows, conv, it = [], False, 0
    while it < opt.max_num_iterations:
        o.linearize(huber)
        o.damp_invert(lam)
        o.schur()
        if prior is not None:
            S, rhs = o.get_S()
            g = b - Hs @ delta_of(o.get_poses(), prior)
            Hd = Hs + lam * np.diag(np.diag(Hs))
            S[ix] += Hd
            rhs[cols] += g
            o.set_S(S, rhs)
        o.solve_reduced()
        o.backsub()
        o.backup()
        o.update()
        cur = o.cost() + pn() if prior is not None else o.cost()
        model = rho = 0.0
        status = 0
        if not opt.gauss_newton:
            model = o.model_change()
            if prior is not None:
                x = o.get_xy()[0].reshape(-1)[cols]
                model -= g @ x + x @ Hd @ x
            with np.errstate(all="ignore"):
                rho = (cur - prev) * 100.0 / model
            if rho > 0.25:
                status = 0
            else:
                o.revert()
                status = 2
            if rho > 0.5:
                lam = max(1e-10, lam * float(opt.decrease_ratio_lambda))
                status = 1
            elif rho <= 0.25:
                lam = min(100.0, lam * float(opt.increase_ratio_lambda))
        sp, sq = o.step_norms()
        avg_step = (sq + sp) / float(o.N + o.M)
        change = abs(cur - prev)
        conv = avg_step < float(opt.threshold_step_size) or change < float(opt.threshold_cost_change)
        if it >= opt.max_num_iterations - 1:
            conv = False
        rows.append(types.SimpleNamespace(
            iteration_status=status, damping_term=lam, trial_cost=cur, rho=rho, model_change=model,
            abs_step=avg_step, cost=prev if status == 2 else cur, cost_change=0.0 if status == 2 else change))
        prev = cur
        it += 1
        if conv:
            break
    out = rows, conv, o.get_poses(), o.get_points()
    o.close()
    return out


def _linearized(pr, huber, keep_obs=None):
    sub = dict(pr)
    if keep_obs is not None:
        for k in OBS_KEYS:
            sub[k] = np.ascontiguousarray(np.asarray(pr[k])[keep_obs])
    o = O.Oracle(sub)
    o.linearize(huber)
    o.damp_invert(0.0)
    A, a = o.get_A()
    Cm, b = o.get_C()
    pi, pj, W = o.get_pairs()
    o.close()
    return A, a, Cm, b, pi, pj, W


def marg_with_prior(pr, marg, prior, huber=1.0):
    """marg_ref.reference with the old prior (None: without) linearised at the values of pr
    joined to the factors: (H (6K, 6K), b (6K,), noise, kept, L)"""
    marg = np.asarray(marg) != 0
    kept, in_l = marg_ref.plan(pr, marg)
    A, a, Cm, b, pi, pj, W = _linearized(pr, huber, in_l[np.asarray(pr["obs_pt"])])
    ps = np.flatnonzero(np.asarray(pr["pose_fixed"]) == 0)
    qs = np.flatnonzero(np.asarray(pr["pt_fixed"]) == 0)
    sel = in_l[qs]
    remap = np.cumsum(sel) - 1
    N, ML = len(ps), int(sel.sum())
    Hf = cov_ref.full_normal_matrix(A, Cm[sel], remap[pi], pj, W)
    g = np.concatenate([a.reshape(-1), b[sel].reshape(-1)])
    if prior is not None:
        pc = opt_cols(pr, prior)
        Hs = sym_lower(prior["H"])
        Hf[np.ix_(pc, pc)] += Hs
        g[pc] += np.asarray(prior["b"], np.float64) - Hs @ delta_of(np.asarray(pr["pose_T"]), prior)
    cols = lambda js: (6 * np.asarray(js, int)[:, None] + np.arange(6)[None, :]).reshape(-1)
    ik = cols(np.flatnonzero(~marg[ps]))
    im = cols(np.flatnonzero(marg[ps]))
    il = 6 * N + np.arange(3 * ML)
    ie = np.concatenate([im, il])
    if len(ie):   # (i) the joint block at once
        sol = np.linalg.solve(Hf[np.ix_(ie, ie)], np.column_stack([Hf[np.ix_(ie, ik)], g[ie]]))
        H1 = Hf[np.ix_(ik, ik)] - Hf[np.ix_(ik, ie)] @ sol[:, :-1]
        b1 = g[ik] - Hf[np.ix_(ik, ie)] @ sol[:, -1]
    else:
        H1, b1 = Hf[np.ix_(ik, ik)].copy(), g[ik].copy()
    ip = np.arange(6 * N)   # (ii) the landmarks by their 3x3 inverses, the marked poses by Cholesky
    S, r = Hf[np.ix_(ip, ip)].copy(), g[ip].copy()
    for i in range(ML):
        c = 6 * N + 3 * i + np.arange(3)
        V = Hf[np.ix_(ip, c)] @ np.linalg.inv(Hf[np.ix_(c, c)])
        S -= V @ Hf[np.ix_(c, ip)]
        r -= V @ g[c]
    H2, b2 = S[np.ix_(ik, ik)], r[ik]
    if len(im):
        cf = scipy.linalg.cho_factor(S[np.ix_(im, im)], lower=True)
        H2 = H2 - S[np.ix_(ik, im)] @ scipy.linalg.cho_solve(cf, S[np.ix_(im, ik)])
        b2 = b2 - S[np.ix_(ik, im)] @ scipy.linalg.cho_solve(cf, r[im])
    noise = max(marg_ref.rel_diff(H2, H1), marg_ref.rel_diff(b2, b1))
    return H1, b1, noise, kept, in_l


def cov_with_prior(pr, prior, huber=1.0):
    """(cov_pose [n_pose, 6, 6], cov_pt [n_pt, 3, 3], noise) in user order (fixed members and
    never-observed landmarks zero): the diagonal blocks of the inverse of the full normal
    matrix with the prior's H on its pose block, by the two routes of cov_ref"""
    A, a, Cm, b, pi, pj, W = _linearized(pr, huber)
    ps = np.flatnonzero(np.asarray(pr["pose_fixed"]) == 0)
    qs = np.flatnonzero(np.asarray(pr["pt_fixed"]) == 0)
    seen = np.bincount(pr["obs_pt"], minlength=len(pr["pt_fixed"]))[qs] > 0
    remap = np.cumsum(seen) - 1
    Hf = cov_ref.full_normal_matrix(A, Cm[seen], remap[pi], pj, W)
    if prior is not None:
        pc = opt_cols(pr, prior)
        Hf[np.ix_(pc, pc)] += sym_lower(prior["H"])
    cp, cq, noise = cov_ref.blocks_two_ways(Hf, len(ps), int(seen.sum()))
    full_p = np.zeros((len(pr["pose_fixed"]), 6, 6))
    full_q = np.zeros((len(pr["pt_fixed"]), 3, 3))
    full_p[ps] = cp
    full_q[qs[seen]] = cq
    return full_p, full_q, noise


def reduced_window(pr, marg):
    """-> (problem without the marked poses and the landmarks of L, with the observations
    that are left; kept poses re-indexed in it; old index of its poses; of its points)"""
    marg = np.asarray(marg) != 0
    kept, in_l = marg_ref.plan(pr, marg)
    assert not (marg & (np.asarray(pr["pose_fixed"]) != 0)).any()
    keep_p, keep_q = np.flatnonzero(~marg), np.flatnonzero(~in_l)
    new_p = np.cumsum(~marg) - 1
    new_q = np.cumsum(~in_l) - 1
    ko = ~in_l[np.asarray(pr["obs_pt"])]
    assert not marg[np.asarray(pr["obs_pose"])[ko]].any()   # a fixed point seen by a marked pose
    sub = dict(pr)
    sub["pose_T"] = np.asarray(pr["pose_T"])[keep_p].copy()
    sub["pose_fixed"] = np.asarray(pr["pose_fixed"])[keep_p].copy()
    sub["pt_X"] = np.asarray(pr["pt_X"])[keep_q].copy()
    sub["pt_fixed"] = np.asarray(pr["pt_fixed"])[keep_q].copy()
    sub["obs_cam"] = np.asarray(pr["obs_cam"])[ko].copy()
    sub["obs_pose"] = new_p[np.asarray(pr["obs_pose"])[ko]].astype(np.int32)
    sub["obs_pt"] = new_q[np.asarray(pr["obs_pt"])[ko]].astype(np.int32)
    sub["obs_uv"] = np.asarray(pr["obs_uv"])[ko].copy()
    return sub, new_p[kept].astype(np.int32), keep_p, keep_q


def gn_step(pr, prior, huber=1.0):
    """one Gauss-Newton step at lambda = 0 on the host, two routes: (poses, points, noise)
    after the step, by the oracle's LDL^T and by numpy.linalg.solve on the reduced system"""
    out = []
    for route in (0, 1):
        o = O.Oracle(pr)
        o.linearize(huber)
        o.damp_invert(0.0)
        o.schur()
        S, rhs = o.get_S()
        if prior is not None:
            cols = opt_cols(pr, prior)
            Hs = sym_lower(prior["H"])
            S[np.ix_(cols, cols)] += Hs
            rhs[cols] += np.asarray(prior["b"], np.float64) - Hs @ delta_of(o.get_poses(), prior)
            o.set_S(S, rhs)
        o.solve_reduced()
        if route == 1:
            o.set_x(np.linalg.solve(S, rhs))
        o.backsub()
        o.update()
        out.append((o.get_poses(), o.get_points()))
        o.close()
    noise = max(marg_ref.rel_diff(out[1][0], out[0][0]), marg_ref.rel_diff(out[1][1], out[0][1]))
    return out[0][0], out[0][1], noise


def random_prior(pr, poses, seed, rows=None, c="zero", tangent=1e-2, strength=1.0):
    """A seeded prior on `poses`: H = J^T J from a random J with fewer rows than columns
    (singular), scaled to the size of the problem's own A blocks so that neither side
    drowns the other; b random; T_lin = the problem's poses moved by exp of a `tangent`-sized
    step.  strength multiplies H and b."""
    from bundle_adjustment_solver_amd.solver import prior_constant
    rng = np.random.default_rng(seed)
    poses = np.asarray(poses, np.int32)
    n = 6 * len(poses)
    rows = max(1, n - 3) if rows is None else rows
    A = _linearized(pr, 1.0)[0]
    scale = np.sqrt(np.abs(A).max())
    d = np.tile(np.r_[np.ones(3), np.full(3, 0.1)], len(poses))   # rotations weigh less in A too
    J = rng.standard_normal((rows, n)) * scale * 0.3 * np.sqrt(strength) * d[None, :]
    H = J.T @ J
    b = J.T @ rng.standard_normal(rows) * 1e-2 * scale * np.sqrt(strength)
    T = np.asarray(pr["pose_T"], np.float64)
    T_lin = np.stack([compose(se3_exp(tangent * rng.standard_normal(6) / np.sqrt(6)), T[q]) for q in poses])
    out = dict(poses=poses, H=H, b=b, T_lin=T_lin, c=0.0)
    if c == "constant":
        out["c"] = prior_constant(H, b)
    return out
