"""Host tests of the reference for the relative-pose factors (no GPU): its first-order
Jacobians against central differences, its loop without factors against the oracle's own, and
the accept / reject coverage of the parity cases the GPU tests run."""
import numpy as np
import pytest

from bundle_adjustment_solver_amd.solver import prior_delta, relative_residual
from oracle import oracle_py as O

import prior_ref
import rel_cases
import rel_ref
from prior_ref import compose, se3_exp


def _numeric_jacobians(T_j, T_k, Z, h=1e-6):
    """central differences of r = se3_log(T_j T_k^-1 Z^-1) in the tangents of T <- exp(xi) T"""
    Jj, Jk = np.zeros((6, 6)), np.zeros((6, 6))
    for c in range(6):
        e = np.zeros(6)
        e[c] = h
        Jj[:, c] = (relative_residual(compose(se3_exp(e), T_j), T_k, Z) -
                    relative_residual(compose(se3_exp(-e), T_j), T_k, Z)) / (2 * h)
        Jk[:, c] = (relative_residual(T_j, compose(se3_exp(e), T_k), Z) -
                    relative_residual(T_j, compose(se3_exp(-e), T_k), Z)) / (2 * h)
    return Jj, Jk


@pytest.mark.parametrize("size", [0.0, 0.008, 0.06])
def test_first_order_jacobians_against_central_differences(size):
    """Exact at r = 0 (1e-8 asserted, 1e-10 measured: the rounding of a central difference with
    step 1e-6); away from it the error is the dropped left-Jacobian correction, of first order
    in |r|: asserted below 2 |r|.  Measured on these poses: dr/dxi_j 2.6e-3 and dr/dxi_k 5.6e-3 at
    |r| = 0.008, 2.0e-2 and 4.2e-2 at |r| = 0.06 (the issue, on other poses, gives 0.005 and 0.03)."""
    rng = np.random.default_rng(11)
    T_j = se3_exp(np.r_[rng.standard_normal(3), 0.7 * rng.standard_normal(3)])
    T_k = se3_exp(np.r_[rng.standard_normal(3), 0.7 * rng.standard_normal(3)])
    d = rng.standard_normal(6)
    d *= size / np.sqrt(d @ d)
    # r = se3_log(E Z^-1) = d  <=>  Z = exp(-d) E
    Z = compose(se3_exp(-d), compose(T_j, rel_ref.inverse12(T_k)))
    r = relative_residual(T_j, T_k, Z)
    assert abs(np.sqrt(r @ r) - size) <= 1e-12
    # the residual is the prior's delta with T_lin = Z T_k
    assert np.abs(r - prior_delta(T_j, compose(Z, T_k))).max() <= 1e-13
    Jj, Jk = rel_ref.jacobians(T_j, T_k, Z)
    Nj, Nk = _numeric_jacobians(T_j, T_k, Z)
    ej, ek = np.abs(Jj - Nj).max(), np.abs(Jk - Nk).max()
    print("|r| = %g: |J_j - numeric| = %.3e, |J_k - numeric| = %.3e" % (size, ej, ek))
    tol = 1e-8 if size == 0.0 else 2.0 * size
    assert ej <= tol and ek <= tol


def test_dense_factors_are_j_transpose_omega_j():
    """H = J^T Omega J and g = -J^T Omega r over the stacked Jacobians, fixed poses dropped"""
    name, _, pr, rels = rel_cases.parity_cases()[0]
    T = np.asarray(pr["pose_T"], np.float64)
    H, g = rel_ref.dense_factors(pr, T, rels)
    jopt = rel_ref.opt_index(pr)
    N = int((jopt >= 0).sum())
    H2, g2 = np.zeros_like(H), np.zeros_like(g)
    for f in range(rel_ref.n_factors(rels)):
        j, k = int(rels["j"][f]), int(rels["k"][f])
        J = np.zeros((6, 6 * N))
        Jj, Jk = rel_ref.jacobians(T[j], T[k], rels["Z"][f])
        if jopt[j] >= 0:
            J[:, 6 * jopt[j]:6 * jopt[j] + 6] = Jj
        if jopt[k] >= 0:
            J[:, 6 * jopt[k]:6 * jopt[k] + 6] = Jk
        Om = prior_ref.sym_lower(rels["Omega"][f])
        H2 += J.T @ Om @ J
        g2 -= J.T @ Om @ relative_residual(T[j], T[k], rels["Z"][f])
    assert np.abs(H - H2).max() <= 1e-12 * np.abs(H2).max()
    assert np.abs(g - g2).max() <= 1e-12 * np.abs(g2).max()
    assert np.abs(H - H.T).max() <= 1e-14 * np.abs(H).max()


def test_reference_loop_without_factors_is_the_oracle(built):
    pr = rel_cases.parity_cases()[0][2]
    opt = O.make_options(**rel_cases.FIXED)
    o = O.Oracle(pr)
    orows, oconv = o.solve(opt)
    rows, conv, T, X = rel_ref.lm_with_relatives(pr, None, opt)
    assert len(rows) == len(orows) == rel_cases.ITERS and conv == oconv
    for a, b in zip(rows, orows):
        assert a.iteration_status == b.iteration_status
        assert a.damping_term == b.damping_term
        assert abs(a.trial_cost - b.trial_cost) <= 1e-12 * abs(b.trial_cost)
    assert np.abs(T - o.get_poses()).max() <= 1e-12 and np.abs(X - o.get_points()).max() <= 1e-12


def test_reference_loop_accepts_and_rejects_on_every_parity_case(built):
    """otherwise the reject path of the kernel (no new linearisation, the same off-diagonal
    blocks back into the reset image) is not exercised; and every case carries what the issue
    asks for: a chain, a non-adjacent pair, a fixed j or k, a duplicated pair"""
    kinds = set()
    for name, _, pr, rels in rel_cases.parity_cases():
        rows = rel_ref.lm_with_relatives(pr, rels, O.make_options(**rel_cases.FIXED))[0]
        st = {r.iteration_status for r in rows}
        print(name, [r.iteration_status for r in rows])
        assert 2 in st and (0 in st or 1 in st), (name, st)
        fx = np.asarray(pr["pose_fixed"]) != 0
        pairs = list(zip(rels["j"].tolist(), rels["k"].tolist()))
        assert len(set(pairs)) < len(pairs)
        assert any(abs(j - k) > 1 and not fx[j] and not fx[k] for j, k in pairs)
        kinds |= {"j" for j, k in pairs if fx[j]} | {"k" for j, k in pairs if fx[k]}
        r = rel_ref.residuals(np.asarray(pr["pose_T"]), rels)
        assert min(np.abs(x).max() for x in r) > 1e-4
    assert kinds == {"j", "k"}
