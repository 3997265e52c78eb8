"""Host tests of the Sim(3) arithmetic of the library (csrc/ba_sim3_fn.h through the host-only
entries ba_sim3_exp / ba_sim3_log / ba_sim3_adjoint), of the Sim(3) reference (sim3_ref.py) and
of the scenes the GPU tests compare trajectories on (sim3_cases.py).  No GPU.

(a) exp, log and Ad7 of the library against scipy.linalg.expm / logm of the 4x4 matrix on a
    grid of theta x sigma with |v| <= 2, 1e-11 absolute.  The grid holds a point on each side of
    every switch of sim3_W_coef (|z|^2 = sigma^2 + theta^2 = 0.25; theta = 0.05 beyond it) and
    of the Rodrigues coefficients (theta = 1e-7).  Measured maximum: 1.3e-14.
(b) the round trip log(exp(xi)), Ad7 against vee(S X S^-1), and the first-order property
    r(exp(x_j) S_j, exp(x_k) S_k) = r + x_j - Ad7(E) x_k by finite differences.
(c) fitness of the scenes: every gain ratio of the reference at least 0.1 relative away from
    0.25 and 0.5, every iteration moves chi-square by at least 1e-6 relative, statuses 0, 1 and 2
    all occur; the noise-free scenes reach the truth to 1e-8; the stop scene stops early.
"""
import itertools

import numpy as np
import pytest

from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import sim3_adjoint, sim3_exp, sim3_log

import sim3_cases as cases
import sim3_ref

THETAS = [0.0, 1e-12, 0.9e-7, 1e-7, 1.1e-7, 1e-4, 1e-2, 0.049, 0.051, 0.3, 0.499, 0.501, 1.0, 3.0]
SIGMAS = [0.0, 1e-12, 1e-7, 1e-4, 1e-2, 0.3, 0.499, 0.501, 0.7]
SIGMAS = SIGMAS + [-s for s in SIGMAS[1:]]
# on the circle |z| = 0.5 and on the line theta = 0.05 beyond it: a point on each side
EDGES = [(0.3, 0.3999), (0.3, 0.4001), (0.4, -0.2999), (0.4, -0.3001), (0.0499, 0.6), (0.0501, 0.6),
         (0.0499, -0.6), (0.0501, -0.6), (0.0499, 0.4974), (0.0499, 0.4976)]


def grid():
    rng = np.random.default_rng(5)
    for th, sg in list(itertools.product(THETAS, SIGMAS)) + EDGES:
        for _ in range(2):
            ax = rng.standard_normal(3)
            v = rng.standard_normal(3)
            yield np.r_[v * (2.0 * rng.random() / np.linalg.norm(v)), th * ax / np.linalg.norm(ax), sg]


def test_exp_log_adjoint_match_expm_logm_on_the_grid(built):
    worst = dict(exp=0.0, log=0.0, log_of_ref=0.0, Ad=0.0)
    for xi in grid():
        S, Sr = sim3_exp(xi), sim3_ref.exp(xi)
        worst["exp"] = max(worst["exp"], np.abs(S - Sr).max())
        worst["log"] = max(worst["log"], np.abs(sim3_log(S) - sim3_ref.log(S)).max())
        worst["log_of_ref"] = max(worst["log_of_ref"], np.abs(sim3_log(Sr) - xi).max())
        worst["Ad"] = max(worst["Ad"], np.abs(sim3_adjoint(S) - sim3_ref.adjoint(S)).max())
    print("maximum absolute error on the grid:", worst)
    assert max(worst.values()) <= 1e-11


def test_log_inverts_exp(built):
    worst = 0.0
    for xi in grid():
        worst = max(worst, np.abs(sim3_log(sim3_exp(xi)) - xi).max())
    print("round trip", worst)
    assert worst <= 1e-11


def test_adjoint_is_the_conjugation(built):
    """column i of Ad7(S) = vee(S hat(e_i) S^-1)"""
    rng = np.random.default_rng(6)
    for _ in range(20):
        S = sim3_exp(np.r_[rng.standard_normal(3), 0.8 * rng.standard_normal(3), 0.5 * rng.standard_normal()])
        M = sim3_ref.mat(S)
        want = np.array([sim3_ref.vee(M @ sim3_ref.hat(e) @ np.linalg.inv(M)) for e in np.eye(7)]).T
        assert np.abs(sim3_adjoint(S) - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_jacobians_are_first_order(built):
    """r(exp(x_j) S_j, exp(x_k) S_k) = r + x_j - Ad7(E) x_k up to |x| (|r| + |x|): the left
    Jacobian of the logarithm is I + ad(r) / 2 + ..., |ad(r)| <= 2 |r|, once for each pose"""
    rng = np.random.default_rng(7)
    for _ in range(20):
        Sj = sim3_exp(np.r_[rng.standard_normal(3), 0.5 * rng.standard_normal(3), 0.3 * rng.standard_normal()])
        Sk = sim3_exp(np.r_[rng.standard_normal(3), 0.5 * rng.standard_normal(3), 0.3 * rng.standard_normal()])
        E = sim3_ref.from_mat(sim3_ref.E_of(Sj, Sk))
        Z = sim3_ref.compose(sim3_ref.exp(-1e-3 * rng.standard_normal(7)), E)
        r = sim3_ref.residual(Sj, Sk, Z)
        xj, xk = 1e-6 * rng.standard_normal(7), 1e-6 * rng.standard_normal(7)
        moved = sim3_ref.residual(sim3_ref.compose(sim3_ref.exp(xj), Sj), sim3_ref.compose(sim3_ref.exp(xk), Sk), Z)
        err = np.linalg.norm(moved - (r + xj - sim3_adjoint(E) @ xk))
        x = np.linalg.norm(xj) + np.linalg.norm(sim3_adjoint(E) @ xk)
        assert err <= 3.0 * x * (np.linalg.norm(r) + x) + 1e-14, (err, x, np.linalg.norm(r))


@pytest.mark.parametrize("name", cases.TRAJECTORY)
def test_trajectory_scene_is_fit(name):
    g = cases.scene(name)
    rows, conv, _ = cases.reference(name)
    assert len(rows) == cases.SCENES[name][2] and not conv
    prev = sim3_ref.chi2(g["pose_S"], g["rels"])
    gn = bool(cases.SCENES[name][1].get("gauss_newton"))
    for it, r in enumerate(rows):
        change = abs(prev - r.trial_cost) / prev
        margin = np.inf if gn else min(abs(r.rho - 0.25) / 0.25, abs(r.rho - 0.5) / 0.5)
        print("%s it %d status %d rho %.4f margin %.3f relative change %.3e"
              % (name, it, r.iteration_status, r.rho, margin, change))
        assert margin >= 0.1 and change >= 1e-6
        prev = r.cost


def test_every_status_occurs():
    seen = set()
    for name in cases.TRAJECTORY:
        seen |= {r.iteration_status for r in cases.reference(name)[0]}
    assert seen == {0, 1, 2}
    st = [r.iteration_status for r in cases.reference("g60")[0]]   # rejections, then accepted steps
    assert 2 in st and any(s != 2 for s in st[st.index(2):]) and {0, 1, 2} <= set(st), st


def test_sizes_straddle_the_tiles_and_one_linearisation_workgroup():
    counts = [len(cases.scene(n)["rels"]["j"]) for n in ("g30_31", "g30_32", "g30_33")]
    assert counts == [cases.FPB - 1, cases.FPB, cases.FPB + 1]
    sizes = {n: int((cases.scene(n)["pose_fixed"] == 0).sum()) for n in ("g2", "n4", "n5", "n9", "n10")}
    assert sizes == dict(g2=1, n4=4, n5=5, n9=9, n10=10)
    assert 7 * int((cases.scene("g60")["pose_fixed"] == 0).sum()) > 96


def test_scenes_hold_both_orientations_a_twin_fixed_ends_and_scale_drift():
    g = cases.scene("g60")
    j, k, fx = g["rels"]["j"], g["rels"]["k"], g["pose_fixed"]
    assert (j > k).any() and (j < k).any()
    pairs = list(zip(j.tolist(), k.tolist()))
    assert any((b, a) in pairs for a, b in pairs)
    assert any(fx[a] and not fx[b] for a, b in pairs) and any(fx[b] and not fx[a] for a, b in pairs)
    assert np.all(g["truth"][:, 12] == 1.0) and np.abs(np.log(g["pose_S"][:, 12])).max() > 0.1


@pytest.mark.parametrize("name", sorted(cases.EXACT))
def test_reference_reaches_the_truth_without_noise(name):
    g = cases.scene(name)
    assert sim3_ref.pose_distance(g["pose_S"], g["truth"]) > 1e-4
    rows, _, S = sim3_ref.lm(g, make_options(max_iter=8, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4))
    err = sim3_ref.pose_distance(S, g["truth"])
    print(name, "distance to the truth", err, "chi2", rows[-1].cost)
    assert err <= 1e-8


def test_stop_scene_stops_early():
    rows, conv, _ = cases.stop_reference()
    print("the reference stops after", len(rows), "iterations")
    assert conv and 2 <= len(rows) < cases.STOP["opt"]["max_iter"]
