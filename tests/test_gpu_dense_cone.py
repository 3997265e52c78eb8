"""The cone sweep of the reduced solve (k_chol_back_cone: the workgroup of a leaf tile solves
its own chain of ancestor tiles, no hand-off between workgroups; csrc/ba_dense_tile.inc,
lists: csrc/ba_dense_sched.cpp dense_cone_lists) against the sweeps it replaces
(BA_DENSE_CONE=0: k_chol_back_flow, or k_chol_back per level under a captured graph).  A step
of a cone is the gather and the block back substitution of k_chol_back operation by
operation, so every comparison here is BIT identity, not a tolerance."""
import os

import numpy as np
import pytest

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import BaProblem

pytestmark = pytest.mark.gpu


class environment:
    """The BA_* variables of a handle: every handle reads them once, at its creation."""

    def __init__(self, **env):
        self.env = env

    def __enter__(self):
        for k, v in self.env.items():
            os.environ[k] = v

    def __exit__(self, *exc):
        for k in self.env:
            os.environ.pop(k, None)


def block_tridiagonal_spd(tiles, nb, rng, shift=None):
    """SPD, non-zero exactly on the block tridiagonal of nb x nb tiles; the last tile is
    five columns short (padding columns in the dense image).  shift: what is added to the
    diagonal (default 4 nb; 0 leaves a matrix that need not be definite)."""
    shift = 4.0 * nb if shift is None else shift
    n = tiles * nb - 5
    A = np.zeros((n, n))
    for t in range(tiles):
        a, b = t * nb, min(n, (t + 1) * nb)
        Q = rng.standard_normal((b - a, b - a))
        A[a:b, a:b] = Q @ Q.T + shift * np.eye(b - a)
        if t + 1 < tiles:
            c = min(n, (t + 2) * nb)
            A[b:c, a:b] = rng.standard_normal((c - b, b - a))
            A[a:b, b:c] = A[b:c, a:b].T
    return A, rng.standard_normal(n)


@pytest.fixture(scope="module")
def systems():
    rng = np.random.default_rng(41)
    return {(tiles, nb): block_tridiagonal_spd(tiles, nb, rng)
            for nb in (32, 64) for tiles in (2, 3, 4, 5, 9, 17, 40)}


@pytest.mark.parametrize("tail", [None, "0"], ids=["tail", "no_tail"])
@pytest.mark.parametrize("nb", [32, 64])
def test_stand_alone_solve_is_bit_identical_to_the_dataflow_sweep(built, systems, nb, tail):
    """ba_dense_spd_solve on block-tridiagonal SPD systems of 2, 3, 4, 5, 9, 17 and 40 tiles
    (odd-even reduction: 2 .. 6 levels; with the tail the systems of 2 and 3 tiles at tile
    order 32 have no non-tail position and launch no sweep at all): x with the cone sweep
    equals x with BA_DENSE_CONE=0 bit for bit, at both tile orders, with k_chol_tail and
    with BA_DENSE_TAIL=0, and for a second solve on the same handle; and it solves the
    system (1e-10 relative, the bound of test_dense_spd_solve)."""
    env = {"BA_DENSE_NB": str(nb)}
    if tail is not None:
        env["BA_DENSE_TAIL"] = tail
    with environment(**env):
        cone = BaProblem(0)
    with environment(BA_DENSE_CONE="0", **env):
        flow = BaProblem(0)
    for tiles in (2, 3, 4, 5, 9, 17, 40):
        A, b = systems[(tiles, nb)]
        ref = np.linalg.solve(A, b)
        x0, _ = flow.dense_spd_solve(A, b)
        assert np.abs(x0 - ref).max() <= 1e-10 * np.abs(ref).max(), tiles
        for again in range(2):
            x1, _ = cone.dense_spd_solve(A, b)
            assert (x1 == x0).all(), (tiles, again, np.abs(x1 - x0).max())


def window_scene(kind, n_pose):
    if kind == "c1":
        return scenes.test_ba_scene()
    if kind == "mono":
        return scenes.synthetic_ba_scene(n_pose, 60 * n_pose, 10, False, seed=51)
    return scenes.synthetic_ba_scene(n_pose, 75 * n_pose, 5, True, seed=52)


def make_gpu(pr):
    p = BaProblem(0)
    p.set_cameras(pr["cam_intr"], pr["cam_T"])
    p.set_poses(pr["pose_T"], pr["pose_fixed"])
    p.set_points(pr["pt_X"], pr["pt_fixed"])
    p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
    p.finalize()
    return p


@pytest.mark.parametrize("kind,n_pose", [("mono", 12), ("mono", 40), ("stereo", 12), ("stereo", 40), ("c1", 0)])
def test_lm_trajectory_is_bit_identical_with_and_without_the_cone_sweep(built, kind, n_pose):
    """Ten LM iterations of mono and stereo window scenes of 12 poses (the whole reduced
    system is the tail: no sweep) and 40 poses (8 tiles, 5 of them non-tail) and of C1: log
    rows and final parameters agree bit for bit between the default, BA_DENSE_CONE=0, and
    both under BA_GRAPH=1 (where BA_DENSE_CONE=0 means one k_chol_back per level)."""
    pr = scenes.scaled_problem(window_scene(kind, n_pose))
    runs = []
    for env in ({}, {"BA_DENSE_CONE": "0"}, {"BA_GRAPH": "1"}, {"BA_GRAPH": "1", "BA_DENSE_CONE": "0"}):
        with environment(**env):
            g = make_gpu(pr)
        rows, _ = g.solve(make_options(max_iter=10, thr_step=0, thr_cost=0))
        assert g.get_dropped_pivots() == 0
        runs.append(([(r.iteration_status, r.cost, r.trial_cost, r.damping_term) for r in rows],
                     g.get_poses().copy(), g.get_points()[0].copy()))
    assert len(runs[0][0]) == 10
    for other in runs[1:]:
        assert other[0] == runs[0][0]
        assert (other[1] == runs[0][1]).all() and (other[2] == runs[0][2]).all()


def test_the_knob_reaches_the_launch_plan(built, capfd):
    """The comparisons above compare two different sweeps: on the 40-pose stereo scene (a
    chain of 8 tiles) the plan printed under BA_PLAN_STATS takes the cone sweep by default
    and not with BA_DENSE_CONE=0."""
    pr = scenes.scaled_problem(window_scene("stereo", 40))
    said = []
    for env in ({}, {"BA_DENSE_CONE": "0"}):
        capfd.readouterr()
        with environment(BA_PLAN_STATS="1", **env):
            make_gpu(pr)
        said.append([l for l in capfd.readouterr().err.splitlines() if l.startswith("dense cone sweep:")])
    assert len(said[0]) == 1 and "taken instead" in said[0][0], said
    assert len(said[1]) == 1 and "not taken" in said[1][0], said
