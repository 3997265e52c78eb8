"""GPU tests of ba_covariance (BaProblem.covariance, ComputeCovariance): pose and
landmark blocks of the inverse of the solver's normal matrix, read off the tile
Cholesky of the reduced camera system (csrc/ba_cov.hip).

Reference of every case: numpy fp64 on the host.  stage_linearize(0, huber), then the
full H = [[A, W], [W^T, C]] from get_A / get_C / get_pairs and numpy.linalg.inv(H); its
pose and point diagonal blocks are the expected outputs (so the landmark formula and the
off-diagonal pose blocks it needs are checked, not just S^-1; in stereo H carries the
last-writer rule of the cross block by construction).

Tolerance: the error of an inverse scales with cond(H) eps.  Per scene the reference is
computed twice — inv(H), and scipy cho_factor / cho_solve on identity columns — and the
largest relative block difference between the two is the reference's own noise (it must
be <= 1e-8, else the scene is unfit); the GPU result has to lie within 10 x that noise
(floor 1e-12 relative), which covers the different elimination order of the tile schedule.

The one-tile scene (mono, 3 poses with 1 fixed: 12 columns + 20 padding columns, 12
optimisable landmarks) has two further FIXED landmarks: with one fixed pose and no fixed
point a monocular problem keeps its scale gauge, H is singular (cond 8e17, Cholesky
fails) and no reference exists; the fixed points remove the gauge (cond 8e5) and leave
the shape — columns, tiles, selected landmarks — as it is.
"""
import numpy as np
import pytest

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import (BaProblem, Camera, FullBundleAdjustmentSolver,
                                                 covariance_to_user_units)

import cov_ref

pytestmark = pytest.mark.gpu

HUBER = 1.0


def make_gpu(pr):
    p = BaProblem(0)
    p.set_cameras(pr["cam_intr"], pr["cam_T"])
    p.set_poses(pr["pose_T"], pr["pose_fixed"])
    p.set_points(pr["pt_X"], pr["pt_fixed"])
    p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
    p.finalize()
    return p


def scene(kind):
    if kind == "onetile":
        sc = scenes.synthetic_ba_scene(n_pose=3, n_pt=14, window=3, stereo=False, seed=7, n_fixed=1)
        sc["pt_fixed"] = np.arange(14) >= 12
        sc["X_init"][12:] = sc["X_true"][12:]
        return sc
    if kind == "mono28":    # 23 free poses = 138 columns = 5 tiles of 32, banded
        return scenes.synthetic_ba_scene(n_pose=28, n_pt=150, window=5, stereo=False, seed=11, n_fixed=5)
    if kind == "stereo12":  # Q1 (last-writer rule of the cross block) active
        return scenes.synthetic_ba_scene(n_pose=12, n_pt=150, window=5, stereo=True, seed=12, n_fixed=5)
    raise KeyError(kind)


_cache = {}


def case(kind):
    """(problem dict, user indices of the free poses / points, reference pose blocks,
    reference point blocks, reference noise, select-all GPU result) — computed once."""
    if kind not in _cache:
        pr = scenes.scaled_problem(scene(kind))
        p = make_gpu(pr)
        p.stage_linearize(0.0, HUBER)
        A, _ = p.get_A()
        Cm, _ = p.get_C()
        pi, pj, W = p.get_pairs()
        H = cov_ref.full_normal_matrix(A, Cm, pi, pj, W)
        cp, cq, noise = cov_ref.blocks_two_ways(H, p.N, p.M_global)
        ps = np.nonzero(pr["pose_fixed"] == 0)[0]
        qs = np.nonzero(pr["pt_fixed"] == 0)[0]
        got = p.covariance(ps, qs, HUBER)
        info = (p.get_dense_info(), p.N, p.covariance_info())
        p.close()
        _cache[kind] = (pr, ps, qs, cp, cq, noise, got, info)
    return _cache[kind]


@pytest.mark.parametrize("kind", ["onetile", "mono28", "stereo12"])
def test_blocks_match_the_host_inverse(built, kind):
    pr, ps, qs, cp, cq, noise, (gp, gq, dropped), (dense, N, _) = case(kind)
    err_p, err_q = cov_ref.rel_block_diff(gp, cp), cov_ref.rel_block_diff(gq, cq)
    print("%s: npad %d fill %.3f  reference noise %.3e  gpu error pose %.3e point %.3e"
          % (kind, dense["npad"], dense["fill"], noise, err_p, err_q))
    assert noise <= 1e-8, "scene unfit: the two host references disagree"
    assert dropped == 0
    assert gp.shape == (ps.size, 6, 6) and gq.shape == (qs.size, 3, 3)
    tol = 10.0 * max(noise, 1e-12)
    assert err_p <= tol and err_q <= tol, (err_p, err_q, tol)
    # blocks of an inverse of an SPD matrix: symmetric to the bit (one MFMA chain per
    # entry, products commute), positive diagonal
    assert np.array_equal(gp, gp.transpose(0, 2, 1)) and np.array_equal(gq, gq.transpose(0, 2, 1))
    assert (np.einsum("nii->ni", gp) > 0).all() and (np.einsum("nii->ni", gq) > 0).all()


def test_shapes_cover_one_tile_and_a_banded_schedule(built):
    """The three scenes of this module: one tile of 32; five banded tiles of 32; and, for
    stereo12, ONE tile of 64 — npad 64 is one tile of 64 or two of 32, and the single level
    of the schedule says which.  So no scene here takes k_cov_solve<64> past its first
    tile: tile order 64 with several tiles, fill-in and long landmarks are the subject of
    test_gpu_covariance_shapes.py."""
    dense, N, _ = case("onetile")[7]
    assert N == 2 and dense["npad"] == 32            # 12 columns + 20 padding columns
    dense, N, _ = case("mono28")[7]
    assert N == 23 and dense["npad"] == 160          # 138 columns, 5 tiles of 32
    assert dense["fill"] < 1.0                       # zero tiles in the schedule
    dense, N, _ = case("stereo12")[7]
    assert N == 7 and dense["npad"] == 64            # 42 columns + 22 padding columns
    assert dense["levels"] == 1 and dense["fill"] == 1.0


def test_more_than_one_column_batch(built, monkeypatch):
    """BA_COV_BATCH=64: four waves (eight poses or twenty points) per batch; mono28 has
    12 pose groups and 30 point groups, so 11 batches — the same bits as in one batch."""
    pr, ps, qs, cp, cq, noise, (gp, gq, _), (_, _, info) = case("mono28")
    assert info["last_batches"] == 1 and info["cols_per_wave"] == 16
    assert 6 * ps.size + 3 * qs.size > 64
    monkeypatch.setenv("BA_COV_BATCH", "64")
    p = make_gpu(pr)
    assert p.covariance_info()["batch_cols"] == 64
    bp, bq, dropped = p.covariance(ps, qs, HUBER)
    assert p.covariance_info()["last_batches"] == 11 and dropped == 0
    p.close()
    assert np.array_equal(bp, gp) and np.array_equal(bq, gq)


def test_selection_order_and_repeats(built):
    pr, ps, qs, _, _, _, (gp, gq, _), _ = case("mono28")
    kp = np.array([17, 9, 4, 9, 0])       # positions in the select-all result: reversed, one repeat
    kq = np.array([149, 80, 33, 80, 2, 1])
    p = make_gpu(pr)
    sp, sq, dropped = p.covariance(ps[kp], qs[kq], HUBER)
    only_p = p.covariance(ps[kp], [], HUBER)
    only_q = p.covariance([], qs[kq], HUBER)
    p.close()
    assert dropped == 0
    assert np.array_equal(sp, gp[kp]) and np.array_equal(sq, gq[kq])
    assert np.array_equal(only_p[0], gp[kp]) and only_p[1].shape == (0, 3, 3)
    assert np.array_equal(only_q[1], gq[kq]) and only_q[0].shape == (0, 6, 6)


def test_two_calls_give_the_same_bits(built):
    pr, ps, qs, _, _, _, (gp, gq, _), _ = case("stereo12")
    p = make_gpu(pr)
    a = p.covariance(ps, qs, HUBER)
    b = p.covariance(ps, qs, HUBER)
    p.close()
    for x, y, z in zip(a[:2], b[:2], (gp, gq)):
        assert np.array_equal(x, y) and np.array_equal(x, z)


def test_never_observed_landmark_has_a_zero_block(built):
    sc = scene("onetile")
    sc["X_init"] = np.vstack([sc["X_init"], [[1.0, 2.0, 8.0]]])
    sc["pt_fixed"] = np.r_[sc["pt_fixed"], False]
    pr = scenes.scaled_problem(sc)
    p = make_gpu(pr)
    cp, cq, dropped = p.covariance([1, 2], [14, 3], HUBER)
    p.close()
    ref_p, ref_q = case("onetile")[6][:2]
    assert dropped == 0
    assert np.array_equal(cq[0], np.zeros((3, 3)))
    assert np.abs(cq[1]).max() > 0
    # the other blocks do not notice the extra landmark
    assert cov_ref.rel_block_diff(cp, ref_p) < 1e-9 and cov_ref.rel_block_diff(cq[1:], ref_q[3:4]) < 1e-9


def _rows(rows):
    keys = ("cost", "cost_change", "average_reprojection_error", "abs_gradient", "abs_step",
            "damping_term", "iteration_status", "rho", "model_change", "trial_cost")
    return [tuple(getattr(r, k) for k in keys) for r in rows]


def test_solve_after_covariance_is_the_solve_without_it(built):
    pr, ps, qs = case("stereo12")[:3]
    opt = make_options(max_iter=6, thr_step=0.0, thr_cost=0.0)
    a, b = make_gpu(pr), make_gpu(pr)
    T0, X0 = a.get_poses(), a.get_points()[0]
    _, _, dropped = a.covariance(ps, qs, 0.37)          # (another Huber threshold than the solve's)
    assert dropped == 0
    assert np.array_equal(a.get_poses(), T0) and np.array_equal(a.get_points()[0], X0)
    ra, ca = a.solve(opt)
    rb, cb = b.solve(opt)
    assert len(ra) == len(rb) == 6 and ca == cb
    assert _rows(ra) == _rows(rb)
    assert np.array_equal(a.get_poses(), b.get_poses())
    assert np.array_equal(a.get_points()[0], b.get_points()[0])
    # ... and the counter of the LM loop's dropped pivots is the loop's own
    assert a.get_dropped_pivots() == b.get_dropped_pivots() == 0
    # after a solve: covariance of the solution, still leaving the state alone
    T1 = a.get_poses()
    c1 = a.covariance(ps[:3], qs[:4], HUBER)
    assert c1[2] == 0 and np.array_equal(a.get_poses(), T1)
    a.close()
    b.close()


def test_facade_returns_user_units_of_the_raw_call(built):
    sc = scenes.test_ba_scene()
    s = FullBundleAdjustmentSolver(0)
    for c in range(sc["intr"].shape[0]):
        s.AddCamera(c, Camera(*sc["intr"][c], pose_this_to_cam0=sc["T_cj"][c]))
    poses, pts = sc["T_wc_init"].copy(), sc["X_init"].copy()
    hp, hq = s.AddPoseArray(poses), s.AddPointArray(pts)
    for j in np.nonzero(sc["pose_fixed"])[0]:
        s.MakePoseFixed(int(hp[j]))
    for c in range(sc["intr"].shape[0]):
        m = sc["obs_cam"] == c
        s.AddObservations(c, hp[sc["obs_pose"][m]], hq[sc["obs_pt"][m]], sc["obs_uv"][m])
    sel_p = [int(hp[k]) for k in (59, 5, 30)]
    sel_q = [int(hq[k]) for k in (0, 650, 333, 0)]
    cov_p, cov_q = s.ComputeCovariance(sel_p, sel_q, sigma_pixel=0.7)
    raw_p, raw_q, dropped = s._problem.covariance(sel_p, sel_q, 1.0)
    exp_p, exp_q = covariance_to_user_units(raw_p, raw_q, 0.7)
    assert dropped == 0 and cov_p.shape == (3, 6, 6) and cov_q.shape == (4, 3, 3)
    assert np.array_equal(cov_p, exp_p) and np.array_equal(cov_q, exp_q)
    assert np.array_equal(cov_q[0], cov_q[3]) and (np.einsum("nii->ni", cov_p) > 0).all()
    with pytest.raises(RuntimeError):
        s.ComputeCovariance([int(hp[0])], [])          # a fixed pose
    with pytest.raises(RuntimeError):
        s.ComputeCovariance([np.eye(4)], [])           # never registered
