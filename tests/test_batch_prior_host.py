"""Host tests of the pose prior of the batch path (no GPU): the reference LM loop of
prior_ref against the oracle's own, the numpy se3 logarithm, the unit conversion, the prior
constant, and the validation of ba_batch_prior_check."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg

from bundle_adjustment_solver_amd import _lib
from bundle_adjustment_solver_amd.solver import (marginal_to_user_units, prior_constant,
                                                 prior_to_scaled_units, se3_log)
from oracle import oracle_py as O

import marg_ref
import prior_ref


@pytest.mark.parametrize("name", ["mono5_m1", "stereo12_m3"])
def test_reference_loop_without_prior_is_the_oracle(built, name):
    pr = marg_ref.build_scene(name)[0]
    opt = O.make_options(max_iter=8, thr_step=0.0, thr_cost=0.0)
    o = O.Oracle(pr)
    orows, oconv = o.solve(opt)
    rows, conv, T, X = prior_ref.lm_with_prior(pr, None, opt)
    assert len(rows) == len(orows) == 8 and conv == oconv
    for a, b in zip(rows, orows):
        assert a.iteration_status == b.iteration_status
        assert a.damping_term == b.damping_term
        assert abs(a.trial_cost - b.trial_cost) <= 1e-12 * abs(b.trial_cost)
        assert abs(a.cost - b.cost) <= 1e-12 * abs(b.cost)
    assert np.abs(T - o.get_poses()).max() <= 1e-12 and np.abs(X - o.get_points()).max() <= 1e-12


def _hat4(x):
    v, w = x[:3], x[3:]
    M = np.zeros((4, 4))
    M[:3, :3] = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
    M[:3, 3] = v
    return M


def _vee4(M):
    return np.r_[M[:3, 3], M[2, 1], M[0, 2], M[1, 0]]


@pytest.mark.parametrize("theta", [0.0, 1e-9, 1e-7, 1e-3, 1.0, 3.0])
def test_se3_log_inverts_se3_exp_and_agrees_with_logm(theta):
    """x = [v; theta * axis] with |v| of the size the solver sees (scaled units, 1e-2, the
    tangent of the parity tests).  se3_exp here is the library's formula, which evaluates
    (1 - cos theta) / theta^2 with a cancellation error of up to ~1 % just above its
    threshold theta = 1e-7; that error moves t by up to 1e-2 * theta * |v| = 1e-11 |v|, which
    is why |v| is not of order one for the round trip.  The logarithm itself is checked
    against scipy.linalg.logm and against the exact exponential (scipy.linalg.expm) at every
    theta.  Tolerance 1e-12 absolute everywhere except theta = 3 (0.14 rad from the
    singularity at pi, 1 / sin theta = 7): measured there |log(exp x) - x| = 1.3e-15 and
    |log - logm| = 4.6e-15, asserted at 1e-14."""
    rng = np.random.default_rng(3)
    axis = rng.standard_normal(3)
    axis /= np.sqrt(axis @ axis)
    x = np.r_[1e-2 * rng.standard_normal(3), theta * axis]
    T12 = prior_ref.se3_exp(x)
    got = se3_log(T12)
    T44 = np.eye(4)
    T44[:3, :3], T44[:3, 3] = T12[:9].reshape(3, 3), T12[9:]
    ref = _vee4(np.real(scipy.linalg.logm(T44)))
    tol = 1e-14 if theta == 3.0 else 1e-12
    print("theta %g: |log(exp x) - x| = %.3g, |log - logm| = %.3g"
          % (theta, np.abs(got - x).max(), np.abs(got - ref).max()))
    assert np.abs(got - x).max() <= tol
    assert np.abs(got - ref).max() <= tol
    assert np.abs(scipy.linalg.expm(_hat4(got)) - T44).max() <= tol


def test_prior_to_scaled_units_inverts_marginal_to_user_units():
    rng = np.random.default_rng(4)
    J = rng.standard_normal((20, 18))
    H, b, c = J.T @ J, rng.standard_normal(18), 3.7
    for sigma in (1.0, 0.37):
        Hu, bu = marginal_to_user_units(H, b, sigma)
        cu = c / (sigma ** 2 * 1e-4)
        H2, b2, c2 = prior_to_scaled_units(Hu, bu, cu, sigma)
        assert np.abs(H2 - H).max() <= 1e-15 * np.abs(H).max()
        assert np.abs(b2 - b).max() <= 1e-15 * np.abs(b).max()
        assert abs(c2 - c) <= 1e-15 * c


def test_prior_constant_zeroes_the_minimum_energy_of_a_singular_prior():
    rng = np.random.default_rng(6)
    J = rng.standard_normal((11, 18))             # rank 11 of 18
    H = J.T @ J
    b = J.T @ rng.standard_normal(11)             # in the range of H: the energy has a minimum
    c = prior_constant(H, b)
    d = np.linalg.lstsq(H, b, rcond=None)[0]
    e_min = d @ H @ d - 2 * b @ d + c
    assert abs(e_min) <= 1e-12 * c and c > 0
    for _ in range(5):                            # and it is the minimum
        dd = d + rng.standard_normal(18)
        assert dd @ H @ dd - 2 * b @ dd + c >= -1e-12 * c
    assert prior_constant(np.zeros((0, 0)), np.zeros(0)) == 0.0


def _check(B, pose_off, pose_fixed, off, pose, T, H, b, c):
    lib = _lib.load()
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    f64 = lambda a: np.ascontiguousarray(a, np.float64)
    pose_off, off, pose = i32(pose_off), i32(off), i32(pose)
    fx = np.ascontiguousarray(pose_fixed, np.uint8)
    T, H, b = f64(T), f64(H), f64(b)
    c = None if c is None else f64(c)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.ba_batch_prior_check(B, ip(pose_off), fx.ctypes.data_as(C.POINTER(C.c_uint8)), ip(off), ip(pose),
                                  dp(T), dp(H), dp(b), dp(c))
    return rc, (lib.ba_last_error() or b"").decode()


def test_prior_check_validation(built):
    """three problems of 4, 3 and 5 poses, the first pose of each fixed; priors on problems
    0 (K = 2) and 2 (K = 3), none on problem 1 (K_p = 0)"""
    pose_off = [0, 4, 7, 12]
    fixed = np.zeros(12, np.uint8)
    fixed[[0, 4, 7]] = 1
    eye = np.r_[np.eye(3).reshape(9), np.zeros(3)]

    def valid():
        return dict(off=[0, 2, 2, 5], pose=[1, 3, 1, 2, 4], T=np.tile(eye, (5, 1)),
                    H=np.r_[np.eye(12).reshape(-1), np.eye(18).reshape(-1)], b=np.zeros(30), c=np.zeros(3))

    def run(**kw):
        a = valid()
        a.update(kw)
        return _check(3, pose_off, fixed, a["off"], a["pose"], a["T"], a["H"], a["b"], a["c"])

    assert run()[0] == 0
    assert run(c=None)[0] == 0
    assert run(off=[0, 0, 0, 0], pose=[], T=[], H=[], b=[])[0] == 0       # every K_p = 0
    bad_H = valid()["H"]
    bad_H[144 + 18 * 3 + 1] = np.nan
    cases = {
        "descending indices": dict(pose=[3, 1, 1, 2, 4]),
        "repeated index": dict(pose=[1, 1, 1, 2, 4]),
        "a fixed pose": dict(pose=[0, 3, 1, 2, 4]),
        "an out-of-range index": dict(pose=[1, 4, 1, 2, 4]),
        "a negative index": dict(pose=[-1, 3, 1, 2, 4]),
        "a NaN in H": dict(H=bad_H),
        "c < 0": dict(c=[0.0, 0.0, -1e-300]),
        "a decreasing offset": dict(off=[0, 2, 1, 5]),
        "a first offset that is not 0": dict(off=[1, 2, 2, 5]),
    }
    for what, kw in cases.items():
        rc, msg = run(**kw)
        assert rc == -1 and msg.startswith("ba_batch_prior_check"), (what, rc, msg)
