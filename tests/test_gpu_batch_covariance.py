"""GPU tests of ba_batch_covariance (BaBatch.covariance, ComputeCovarianceBatch): the pose
and landmark covariance blocks of every problem of a batch in one launch
(k_ba_batch_cov: linearisation, Schur complement, Cholesky and S^-1 in LDS).

Reference, independent of the code under test: the CPU oracle linearises (lambda = 0, the
same Huber threshold), H = [[A, W], [W^T, C]] is assembled from its A / C / pair blocks
(never-observed landmarks left out: they are decoupled and H would be singular) and
inverted twice on the host (cov_ref.blocks_two_ways); the largest relative block
difference between the two inverses is the reference's own noise.

Tolerance: the project's rule of test_gpu_covariance.py — the noise must be <= 1e-8 (else
the scene is unfit) and the GPU blocks lie within 10 x max(noise, 1e-12).

Windows: the smallest that reach every path — 32, 64 and 96 image columns; N = 1 (one
block), N = 3 and 6 (6x6 blocks that straddle a 16-column tile), N = 16 (no padding
column); mono and stereo; fixed poses and fixed points.
"""
import copy

import numpy as np
import pytest

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import (BaBatch, Camera, FullBundleAdjustmentSolver,
                                                 covariance_to_user_units)
from oracle import oracle_py as O

import cov_ref

pytestmark = pytest.mark.gpu

HUBER = 1.0
ROW_FIELDS = ("cost", "cost_change", "average_reprojection_error", "abs_gradient", "abs_step",
              "damping_term", "iteration_status", "rho", "model_change", "trial_cost")


def row_bits(rows):
    return np.array([[getattr(r, f) for f in ROW_FIELDS] for r in rows], float).reshape(-1, len(ROW_FIELDS))


def window(n_pose, n_pt, stereo, seed, n_fixed=2, **kw):
    return scenes.ba_batch_scene(1, n_pose=n_pose, n_pt=n_pt, stereo=stereo, seed=seed,
                                 n_fixed=n_fixed, **kw)[0]


def onetile():
    """the one-tile scene of test_gpu_covariance.py: mono, 3 poses (1 fixed), 2 fixed points"""
    sc = scenes.synthetic_ba_scene(n_pose=3, n_pt=14, window=3, stereo=False, seed=7, n_fixed=1)
    sc["pt_fixed"] = np.arange(14) >= 12
    sc["X_init"][12:] = sc["X_true"][12:]
    return sc


# name -> (scene, optimisable poses, image columns of a batch of its width class)
WINDOWS = {
    "onetile": (onetile, 2, 32),
    "mono5": (lambda: window(5, 37, False, 11), 3, 32),
    "stereo4_3fixed": (lambda: window(4, 29, True, 12, n_fixed=3), 1, 32),
    "mono8": (lambda: window(8, 33, False, 16), 6, 64),
    "stereo12": (lambda: window(12, 40, True, 15), 10, 64),
    "stereo18": (lambda: window(18, 45, True, 13), 16, 96),
    "mono18": (lambda: window(18, 45, False, 17), 16, 96),
}
BY_WIDTH = {w: [k for k, v in WINDOWS.items() if v[2] == w] for w in (32, 64, 96)}


def reference(pr, huber=HUBER):
    """(cov_pose [n_pose, 6, 6], cov_pt [n_pt, 3, 3], noise) of one problem dict from the
    CPU oracle and the host inverse; blocks of fixed members and of never-observed
    landmarks are zero."""
    o = O.Oracle(pr)
    o.linearize(huber)
    o.damp_invert(0.0)
    A, _ = o.get_A()
    Cm, _ = o.get_C()
    pi, pj, W = o.get_pairs()
    o.close()
    ps = np.nonzero(np.asarray(pr["pose_fixed"]) == 0)[0]
    qs = np.nonzero(np.asarray(pr["pt_fixed"]) == 0)[0]
    seen = np.bincount(pr["obs_pt"], minlength=len(pr["pt_fixed"]))[qs] > 0
    remap = np.cumsum(seen) - 1
    assert seen[pi].all()
    H = cov_ref.full_normal_matrix(A, Cm[seen], remap[pi], pj, W)
    cp, cq, noise = cov_ref.blocks_two_ways(H, len(ps), int(seen.sum()))
    full_p = np.zeros((len(pr["pose_fixed"]), 6, 6))
    full_q = np.zeros((len(pr["pt_fixed"]), 3, 3))
    full_p[ps] = cp
    full_q[qs[seen]] = cq
    return full_p, full_q, noise


_cache = {}


def problem(name):
    """(problem dict, reference pose blocks, reference point blocks, noise) — computed once"""
    if name not in _cache:
        pr = scenes.scaled_problem(WINDOWS[name][0]())
        assert int((pr["pose_fixed"] == 0).sum()) == WINDOWS[name][1]
        _cache[name] = (pr,) + reference(pr)
    return _cache[name]


def run(probs, huber=HUBER, points=True, calls=1):
    """BaBatch.covariance of a problem list -> (per-problem (cov_pose, cov_pt, result), image
    columns); with calls > 1 every call must return the bits of the first"""
    b = BaBatch(probs)
    cp, cq, res = b.covariance(huber, points)
    for _ in range(calls - 1):
        cp2, cq2, res2 = b.covariance(huber, points)
        assert np.array_equal(cp, cp2) and (cq is None or np.array_equal(cq, cq2))
        assert [(r.status, r.dropped_pivots) for r in res] == [(r.status, r.dropped_pivots) for r in res2]
    cols = b.info()["image_columns"]
    out = [(b.cov_poses_of(p, cp).copy(), None if cq is None else b.cov_points_of(p, cq).copy(), res[p])
           for p in range(len(probs))]
    b.close()
    return out, cols


def check_blocks(label, pr, got, ref_p, ref_q, noise):
    gp, gq, res = got
    err_p, err_q = cov_ref.rel_block_diff(gp, ref_p), cov_ref.rel_block_diff(gq, ref_q)
    print("%s: reference noise %.3e  gpu error pose %.3e point %.3e" % (label, noise, err_p, err_q))
    assert noise <= 1e-8, "scene unfit: the two host references disagree"
    assert res.status == 0 and res.dropped_pivots == 0
    tol = 10.0 * max(noise, 1e-12)
    assert err_p <= tol and err_q <= tol, (label, err_p, err_q, tol)
    assert np.array_equal(gp, gp.transpose(0, 2, 1)) and np.array_equal(gq, gq.transpose(0, 2, 1))
    pf, qf = np.asarray(pr["pose_fixed"]) != 0, np.asarray(pr["pt_fixed"]) != 0
    assert not gp[pf].any() and not gq[qf].any()        # fixed members: exactly zero
    seen = np.bincount(pr["obs_pt"], minlength=len(qf)) > 0
    assert (np.einsum("nii->ni", gp[~pf]) > 0).all() and (np.einsum("nii->ni", gq[~qf & seen]) > 0).all()


@pytest.fixture(scope="module")
def by_width(built):
    """the three batches of test 1, one per image width, each run twice"""
    out = {}
    for w, names in BY_WIDTH.items():
        got, cols = run([problem(n)[0] for n in names], calls=2)
        assert cols == w
        out.update(zip(names, got))
    return out


@pytest.mark.parametrize("width", [32, 64, 96])
def test_blocks_match_the_host_inverse(by_width, width):
    for name in BY_WIDTH[width]:
        pr, ref_p, ref_q, noise = problem(name)
        check_blocks("%s (N = %d, image %d)" % (name, WINDOWS[name][1], width), pr, by_width[name],
                     ref_p, ref_q, noise)


def test_never_observed_landmark_has_a_zero_block(built):
    sc = window(5, 37, False, 11)
    keep = sc["obs_pt"] != 4
    for k in ("obs_cam", "obs_pose", "obs_pt", "obs_uv"):
        sc[k] = sc[k][keep]
    pr = scenes.scaled_problem(sc)
    ref_p, ref_q, noise = reference(pr)
    (got,), _ = run([pr])
    assert not pr["pt_fixed"][4] and np.array_equal(got[1][4], np.zeros((3, 3)))
    assert not ref_q[4].any() and np.abs(got[1][5]).max() > 0
    check_blocks("mono5 without landmark 4", pr, got, ref_p, ref_q, noise)


def test_position_and_width_independence(by_width):
    names = list(WINDOWS)
    mixed, cols = run([problem(n)[0] for n in names])
    assert cols == 96
    for n, m in zip(names, mixed):
        (alone,), cols1 = run([problem(n)[0]])
        assert cols1 == WINDOWS[n][2]
        for g in (alone, by_width[n]):
            assert np.array_equal(m[0], g[0]) and np.array_equal(m[1], g[1]), n
            assert (g[2].status, g[2].dropped_pivots) == (0, 0)


def test_more_problems_than_cus(built):
    pr = problem("onetile")[0]
    got, _ = run([pr] * 300)
    assert len(got) == 300
    for g in got:
        assert g[2].status == 0 and g[2].dropped_pivots == 0
        assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1])
    assert np.abs(got[0][0]).max() > 0


def test_nothing_visible_changes(built):
    names = ["stereo12", "mono8", "stereo4_3fixed"]
    probs = [problem(n)[0] for n in names]
    opt = make_options(max_iter=5, thr_step=0.0, thr_cost=0.0)
    a, b = BaBatch(probs), BaBatch(probs)
    T0, X0 = a.get_poses(), a.get_points()
    a.covariance(0.37)                      # (another Huber threshold than the solve's)
    assert np.array_equal(a.get_poses(), T0) and np.array_equal(a.get_points(), X0)
    ra, sa = a.solve(opt)
    rb, sb = b.solve(opt)
    for p in range(len(probs)):
        assert np.array_equal(row_bits(ra[p]), row_bits(rb[p])) and len(ra[p]) == 5
        assert (sa[p].n_iter, sa[p].converged, sa[p].status, sa[p].dropped_pivots) == \
            (sb[p].n_iter, sb[p].converged, sb[p].status, sb[p].dropped_pivots)
    T1, X1 = a.get_poses(), a.get_points()
    assert np.array_equal(T1, b.get_poses()) and np.array_equal(X1, b.get_points())
    # after a solve: the covariance of the solution, the values left alone
    cp, cq, res = a.covariance(HUBER)
    assert np.array_equal(a.get_poses(), T1) and np.array_equal(a.get_points(), X1)
    for p, n in enumerate(names):
        pr = copy.copy(probs[p])
        pr["pose_T"], pr["pt_X"] = a.poses_of(p, T1).copy(), a.points_of(p, X1).copy()
        ref_p, ref_q, noise = reference(pr)
        check_blocks("%s at the solved values" % n, pr,
                     (a.cov_poses_of(p, cp), a.cov_points_of(p, cq), res[p]), ref_p, ref_q, noise)
    a.close()
    b.close()


def test_status_codes(built):
    good = problem("stereo18")[0]
    over = scenes.scaled_problem(window(19, 30, True, 21))
    assert int((over["pose_fixed"] == 0).sum()) == 17
    nan = copy.copy(problem("mono5")[0])
    nan["pt_X"] = nan["pt_X"].copy()
    nan["pt_X"][3, 1] = np.nan
    got, _ = run([good, over, nan])
    assert [g[2].status for g in got] == [0, 2, 1]
    for g in got[1:]:
        assert not g[0].any() and not g[1].any()
    (alone,), _ = run([good])
    assert np.array_equal(got[0][0], alone[0]) and np.array_equal(got[0][1], alone[1])
    assert np.abs(alone[0]).max() > 0


def test_points_false_skips_the_landmark_blocks(by_width):
    names = BY_WIDTH[64]
    got, _ = run([problem(n)[0] for n in names], points=False)
    for n, g in zip(names, got):
        assert g[1] is None and g[2].status == 0
        assert np.array_equal(g[0], by_width[n][0])


def _facade_solver(sc):
    s = FullBundleAdjustmentSolver(0)
    for c in range(sc["intr"].shape[0]):
        s.AddCamera(c, Camera(*sc["intr"][c], pose_this_to_cam0=sc["T_cj"][c]))
    hp, hq = s.AddPoseArray(sc["T_wc_init"].copy()), s.AddPointArray(sc["X_init"].copy())
    for j in np.nonzero(sc["pose_fixed"])[0]:
        s.MakePoseFixed(int(hp[j]))
    for c in range(sc["intr"].shape[0]):
        m = sc["obs_cam"] == c
        s.AddObservations(c, hp[sc["obs_pose"][m]], hq[sc["obs_pt"][m]], sc["obs_uv"][m])
    return s


def test_facade_returns_user_units_of_the_raw_call(built):
    scs = [window(5, 37, True, 31), window(7, 41, False, 32)]
    solvers = [_facade_solver(sc) for sc in scs]
    out = FullBundleAdjustmentSolver.ComputeCovarianceBatch(solvers, sigma_pixel=0.7)
    probs = []
    for sv in solvers:
        intr, camT, T_jw, X, pf, qf, ocam, opose, opt, ouv = sv._host_arrays()
        probs.append(dict(cam_intr=intr, cam_T=camT, pose_T=T_jw, pose_fixed=pf, pt_X=X,
                          pt_fixed=qf, obs_cam=ocam, obs_pose=opose, obs_pt=opt, obs_uv=ouv))
    raw, _ = run(probs, huber=1.0)
    assert len(out) == 2
    for sc, (up, uq, res), (rp, rq, _) in zip(scs, out, raw):
        ep, eq = covariance_to_user_units(rp, rq, 0.7)
        assert res.status == 0 and res.dropped_pivots == 0
        assert up.shape == (len(sc["pose_fixed"]), 6, 6) and uq.shape == (len(sc["X_init"]), 3, 3)
        assert np.array_equal(up, ep) and np.array_equal(uq, eq)
        fixed = np.asarray(sc["pose_fixed"]) != 0
        assert fixed.sum() == 2 and not up[fixed].any() and (np.einsum("nii->ni", up[~fixed]) > 0).all()
    pose_only = FullBundleAdjustmentSolver.ComputeCovarianceBatch(solvers, sigma_pixel=0.7, points=False)
    assert pose_only[0][1] is None and np.array_equal(pose_only[0][0], out[0][0])
