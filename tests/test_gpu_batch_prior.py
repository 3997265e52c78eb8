"""GPU tests of the pose prior of the batch path (ba_batch_set_prior as one more factor of
ba_batch_solve, ba_batch_covariance and ba_batch_marginalize) against the host references of
prior_ref.

Tolerances are the project's.  LM trajectories: the rule of test_gpu_full_batch.py (identical
iteration_status, damping_term within 1e-12, cost and trial cost within 1e-7 relative, final
poses and points within 1e-6 relative).  Matrices and one-step comparisons: the rule of
test_gpu_batch_marginalize.py (the two host routes must agree to 1e-8, the GPU lies within
10 x max(noise, 1e-12))."""
import numpy as np
import pytest

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import (BaBatch, BaProblem, Camera,
                                                 FullBundleAdjustmentSolver, Options,
                                                 _T12_to_44, marginal_to_user_units, rigid_inverse)
from oracle import oracle_py as O

import cov_ref
import marg_ref
import prior_ref

pytestmark = pytest.mark.gpu
ITERS = 8
FIXED = dict(max_iter=ITERS, thr_step=0.0, thr_cost=0.0)
ROW_FIELDS = ("cost", "cost_change", "average_reprojection_error", "abs_gradient", "abs_step",
              "damping_term", "iteration_status", "rho", "model_change", "trial_cost")


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def row_bits(rows):
    return np.array([[getattr(r, f) for f in ROW_FIELDS] for r in rows], float).reshape(-1, len(ROW_FIELDS))


def window(n_pose, n_pt, stereo, seed, n_fixed=2):
    return scenes.scaled_problem(scenes.ba_batch_scene(1, n_pose=n_pose, n_pt=n_pt, stereo=stereo, seed=seed,
                                                       n_fixed=n_fixed)[0])


def solve(probs, priors, opt_kw, calls=1):
    """-> per problem (rows, result, poses, points) of a fresh batch; calls > 1 re-solves the
    same start values and requires the bits of the first call"""
    b = BaBatch(probs)
    if priors is not None:
        b.set_prior(priors)
    T0, X0 = b.get_poses(), b.get_points()
    out = None
    for _ in range(calls):
        b.update_values(T0, X0)
        rows, res = b.solve(make_options(**opt_kw))
        T, X = b.get_poses(), b.get_points()
        got = [(rows[p], res[p], b.poses_of(p, T).copy(), b.points_of(p, X).copy()) for p in range(len(probs))]
        if out is not None:
            assert_same_bits(out, got)
        out = got
    b.close()
    return out


def assert_same_bits(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3])
        assert np.array_equal(row_bits(x[0]), row_bits(y[0]), equal_nan=True)
        assert (x[1].status, x[1].n_iter, x[1].dropped_pivots) == (y[1].status, y[1].n_iter, y[1].dropped_pivots)


# ---- 1. LM trajectory parity ------------------------------------------------------------------
# name -> (window, optimisable poses, image columns, prior poses,
#          (seed, strength) of the prior with c = 0 and with c = prior_constant)
PARITY = {
    "stereo4_all": (lambda: window(6, 29, True, 31), 4, 32, [2, 3, 4, 5], ((5, 1.0), (5, 1.0))),
    "mono8_k3": (lambda: window(10, 33, False, 32), 8, 64, [2, 5, 9], ((5, 1.0), (5, 1.0))),
    "stereo16_all": (lambda: window(18, 45, True, 33), 16, 96, list(range(2, 18)), ((5, 1.0), (5, 1.0))),
    # one prior pose against 45 landmarks: only a strong prior makes the loop reject a step, and
    # the two values of c need different ones (chosen on the CPU, from the reference loop alone)
    "stereo16_k1": (lambda: window(18, 45, True, 33), 16, 96, [7], ((5, 1000.0), (2, 100.0))),
}


def parity_cases():
    out = []
    for name, (mk, n_opt, cols, poses, knobs) in PARITY.items():
        pr = mk()
        assert int((pr["pose_fixed"] == 0).sum()) == n_opt
        for c, (seed, strength) in zip(("zero", "constant"), knobs):
            out.append((name, c, cols, pr, prior_ref.random_prior(pr, poses, seed=seed, c=c, strength=strength)))
    return out


@pytest.fixture(scope="module")
def parity(built):
    cases = parity_cases()
    ref = [prior_ref.lm_with_prior(pr, prior, O.make_options(**FIXED)) for _, _, _, pr, prior in cases]
    got = []
    for cols in (32, 64, 96):          # one batch per image width
        idx = [k for k, cs in enumerate(cases) if cs[2] == cols]
        b = BaBatch([cases[k][3] for k in idx])
        assert b.info()["image_columns"] == cols
        b.close()
        got += list(zip(idx, solve([cases[k][3] for k in idx], [cases[k][4] for k in idx], FIXED)))
    got = [g for _, g in sorted(got, key=lambda t: t[0])]
    return cases, ref, got


def check_trajectory(label, got, ref, rtol_cost=1e-7):
    rows, res, T, X = got
    orows, _, oT, oX = ref
    assert res.status == 0 and res.n_iter == len(orows) == res.n_rows == len(rows)
    floor = 1e-12 * abs(orows[0].cost)
    for k, (a, b) in enumerate(zip(rows, orows)):
        print("%s it %d: status %d/%d lambda %.6g/%.6g trial cost %.12g/%.12g rho %.4g/%.4g"
              % (label, k, a.iteration_status, b.iteration_status, a.damping_term, b.damping_term,
                 a.trial_cost, b.trial_cost, a.rho, b.rho))
    for k, (a, b) in enumerate(zip(rows, orows)):
        assert a.iteration_status == b.iteration_status, (label, k)
        assert relerr(a.damping_term, b.damping_term) < 1e-12, (label, k)
        assert abs(a.trial_cost - b.trial_cost) <= rtol_cost * abs(b.trial_cost) + floor, (label, k)
        assert abs(a.cost - b.cost) <= rtol_cost * abs(b.cost) + floor, (label, k)
    assert relerr(T, oT) < 1e-6 and relerr(X, oX) < 1e-6, label


def test_reference_loop_accepts_and_rejects_on_every_case(parity):
    """otherwise the reject path of the kernel (no new linearisation) is not exercised"""
    cases, ref, _ = parity
    for k, cs in enumerate(cases):
        st = {r.iteration_status for r in ref[k][0]}
        assert 2 in st and (0 in st or 1 in st), (cs[0], cs[1], st)


def test_lm_trajectory_matches_the_reference_loop(parity):
    cases, ref, got = parity
    for k, (name, c, _, pr, prior) in enumerate(cases):
        check_trajectory("%s c=%s" % (name, c), got[k], ref[k])
        # the prior matters: without it the first trial cost differs by far more than the tolerance
    free = solve([cases[0][3]], None, FIXED)[0]
    assert relerr(free[0][0].trial_cost, got[0][0][0].trial_cost) > 1e-4


def test_gauss_newton_matches_the_reference_loop(built):
    pr = PARITY["mono8_k3"][0]()
    prior = prior_ref.random_prior(pr, PARITY["mono8_k3"][3], seed=6, c="constant")
    kw = dict(max_iter=4, thr_step=0.0, thr_cost=0.0, gauss_newton=True, lambda0=1e-3)
    ref = prior_ref.lm_with_prior(pr, prior, O.make_options(**kw))
    check_trajectory("gauss-newton", solve([pr], [prior], kw)[0], ref)


# ---- 2. slide consistency ---------------------------------------------------------------------
GN1 = dict(max_iter=1, thr_step=0.0, thr_cost=0.0, gauss_newton=True, lambda0=0.0)


def slide(pr, mk):
    """(kept poses and surviving points after one GN step of the full window, the same of the
    reduced window with the marginal as its prior, the host noise of the two routes, the
    kept poses before the step)"""
    full = BaBatch([pr])
    Hl, bl, kl, res = full.marginalize(mk, 1.0)
    assert res[0].status == 0 and res[0].dropped_pivots == 0
    sub, kp, keep_p, keep_q = prior_ref.reduced_window(pr, mk)
    assert np.array_equal(keep_p[kp], kl[0])
    prior = dict(poses=kp, H=Hl[0].copy(), b=bl[0].copy(), T_lin=sub["pose_T"][kp].copy(), c=0.0)
    full.solve(make_options(**GN1))
    Tf, Xf = full.get_poses()[keep_p], full.get_points()[keep_q]
    full.close()
    Tr, Xr = solve([sub], [prior], GN1)[0][2:]
    # the same two routes on the host
    hH, hb, _, _, _ = prior_ref.marg_with_prior(pr, mk, None)
    hT, hX, n1 = prior_ref.gn_step(pr, None)
    rT, rX, n2 = prior_ref.gn_step(sub, dict(prior, H=hH, b=hb))
    noise = max(n1, n2, marg_ref.rel_diff(rT, hT[keep_p]), marg_ref.rel_diff(rX, hX[keep_q]))
    return (Tf, Xf), (Tr, Xr), noise, sub["pose_T"]


@pytest.mark.parametrize("name", ["mono5_m1", "stereo4_m1"])
def test_slide_consistency(built, name):
    pr, mk, _ = marg_ref.build_scene(name)
    # 16 iterations: converged, but not to the last bit, so that the step the full window
    # still takes (2e-7 mono, 5e-5 stereo) stands clear of the rounding of the values
    conv = solve([pr], None, dict(max_iter=16, thr_step=0.0, thr_cost=0.0))[0]
    pr_conv = dict(pr, pose_T=conv[2], pt_X=conv[3])
    steps = {}
    for label, p in (("perturbed", pr), ("converged", pr_conv)):
        (Tf, Xf), (Tr, Xr), noise, T0 = slide(p, mk)
        eT, eX = marg_ref.rel_diff(Tr, Tf), marg_ref.rel_diff(Xr, Xf)
        print("%s %s: host noise %.3e  gpu difference poses %.3e points %.3e" % (name, label, noise, eT, eX))
        assert noise <= 1e-8, "scene unfit: the two host routes disagree"
        tol = 10.0 * max(noise, 1e-12)
        assert eT <= tol and eX <= tol, (label, eT, eX, tol)
        steps[label] = (np.abs(Tr - T0).max(), np.abs(Tf - T0).max())
    print("%s: steps (reduced, full) %s" % (name, steps))
    assert steps["converged"][1] > 1e-9
    assert steps["converged"][0] <= 10.0 * steps["converged"][1]
    assert steps["converged"][1] < 1e-2 * steps["perturbed"][1]


# ---- 3. chained marginalisation and covariance ------------------------------------------------
def chain_prior(pr, mk, seed, full_rank=False):
    """a prior that touches one marked and two kept poses (or, full rank, every optimisable pose)"""
    opt = np.flatnonzero(np.asarray(pr["pose_fixed"]) == 0)
    marked = [q for q in opt if mk[q]]
    kept = [q for q in opt if not mk[q]]
    poses = sorted(opt if full_rank else [marked[0], kept[0], kept[-1]])
    return prior_ref.random_prior(pr, poses, seed=seed, rows=6 * len(poses) + 4 if full_rank else None)


@pytest.mark.parametrize("name,cols", [("mono8_m2", 64), ("stereo18_m1", 112)])
def test_marginalize_and_covariance_with_a_prior(built, name, cols):
    pr, mk, _ = marg_ref.build_scene(name)
    assert marg_ref.image_columns(pr, mk) == cols
    prior = chain_prior(pr, mk, seed=9)
    assert mk[prior["poses"]].any() and not mk[prior["poses"]].all()
    rH, rb, noise, rkept, _ = prior_ref.marg_with_prior(pr, mk, prior)
    fH, fb, _, _, _ = prior_ref.marg_with_prior(pr, mk, None)
    rp, rq, cnoise = prior_ref.cov_with_prior(pr, prior)
    b = BaBatch([pr])
    b.set_prior([prior])
    Hl, bl, kl, res = b.marginalize(mk, 1.0)
    cp, cq, cres = b.covariance(1.0)
    b.close()
    eH, eb = marg_ref.rel_diff(Hl[0], rH), marg_ref.rel_diff(bl[0], rb)
    ep, eq = cov_ref.rel_block_diff(cp, rp), cov_ref.rel_block_diff(cq, rq)
    print("%s: marg noise %.3e gpu H %.3e b %.3e | cov noise %.3e gpu pose %.3e point %.3e"
          % (name, noise, eH, eb, cnoise, ep, eq))
    assert noise <= 1e-8 and cnoise <= 1e-8, "scene unfit: the two host references disagree"
    assert res[0].status == 0 and res[0].dropped_pivots == 0 and np.array_equal(kl[0], rkept)
    assert cres[0].status == 0 and cres[0].dropped_pivots == 0
    tol = 10.0 * max(noise, 1e-12)
    assert eH <= tol and eb <= tol, (eH, eb, tol)
    ctol = 10.0 * max(cnoise, 1e-12)
    assert ep <= ctol and eq <= ctol, (ep, eq, ctol)
    assert np.array_equal(Hl[0], Hl[0].T)
    # the prior is in the result: it is not the marginal of the window alone
    assert marg_ref.rel_diff(Hl[0], fH) > 1e-6


def test_full_rank_prior_fixes_the_gauge(built):
    """no fixed pose, one camera: S carries the seven gauge directions at lambda = 0 (pivots of
    rounding size, some of them not positive); with a full-rank prior on every pose it is
    positive definite.  (A stereo window is no example: the last-writer rule of its cross
    blocks leaves S regular.)"""
    pr, mk, _ = marg_ref.build_scene("mono16_nofixed_m3")
    assert not pr["pose_fixed"].any()
    prior = chain_prior(pr, mk, seed=10, full_rank=True)
    assert np.linalg.eigvalsh(prior["H"]).min() > 0
    b = BaBatch([pr])
    _, _, free = b.covariance(1.0)
    b.set_prior([prior])
    cp, cq, held = b.covariance(1.0)
    b.close()
    assert free[0].status == 0 and free[0].dropped_pivots > 0
    assert held[0].status == 0 and held[0].dropped_pivots == 0
    rp, rq, noise = prior_ref.cov_with_prior(pr, prior)
    assert noise <= 1e-8
    tol = 10.0 * max(noise, 1e-12)
    assert cov_ref.rel_block_diff(cp, rp) <= tol and cov_ref.rel_block_diff(cq, rq) <= tol


# ---- 4. no behaviour change, determinism ------------------------------------------------------
@pytest.fixture(scope="module")
def trio(built):
    probs = [window(6, 29, True, 41), window(7, 31, False, 42), window(5, 27, True, 43)]
    priors = [prior_ref.random_prior(probs[0], [2, 4], seed=1), None,
              prior_ref.random_prior(probs[2], [2, 3, 4], seed=2, c="constant")]
    return probs, priors


def test_set_then_clear_is_the_never_set_batch(trio):
    probs, priors = trio
    never = solve(probs, None, FIXED)
    b = BaBatch(probs)
    b.set_prior(priors)
    assert b.prior_info()["n_prior"] == 2 and b.prior_info()["total_K"] == 5 and b.prior_info()["device_bytes"] > 0
    b.clear_prior()
    assert b.prior_info() == dict(n_prior=0, total_K=0, device_bytes=0)
    rows, res = b.solve(make_options(**FIXED))
    T, X = b.get_poses(), b.get_points()
    b.close()
    got = [(rows[p], res[p], b.poses_of(p, T), b.points_of(p, X)) for p in range(3)]
    assert_same_bits(never, got)


def test_problem_without_prior_between_two_with(trio):
    probs, priors = trio
    got = solve(probs, priors, FIXED)
    assert_same_bits([got[1]], solve([probs[1]], None, FIXED))


def test_position_independence_and_repeats(trio):
    probs, priors = trio
    alone = solve([probs[0]], [priors[0]], FIXED, calls=3)
    filler, fp = [probs[1], probs[2], probs[1], probs[2]], [None, priors[2], None, None]
    first = solve([probs[0]] + filler, [priors[0]] + fp, FIXED)
    last = solve(filler + [probs[0]], fp + [priors[0]], FIXED)
    assert_same_bits(alone, [first[0]])
    assert_same_bits(alone, [last[4]])
    assert not np.array_equal(alone[0][2], solve([probs[0]], None, FIXED)[0][2])


def test_prior_on_a_problem_over_the_limit_is_ignored(trio):
    probs, priors = trio
    big = window(20, 30, False, 44, n_fixed=2)            # 18 optimisable poses: status 2
    pb = prior_ref.random_prior(big, [2, 3], seed=3)
    got = solve([probs[0], big, probs[2]], [priors[0], pb, priors[2]], FIXED)
    assert got[1][1].status == 2 and np.array_equal(got[1][2], big["pose_T"])
    ref = solve([probs[0], probs[2]], [priors[0], priors[2]], FIXED)
    assert_same_bits(ref, [got[0], got[2]])


def test_zero_prior_changes_nothing_but_the_sign_of_a_zero(trio):
    probs, _ = trio
    pr = probs[0]
    zero = dict(poses=np.array([2, 3, 5], np.int32), H=np.zeros((18, 18)), b=np.zeros(18),
                T_lin=pr["pose_T"][[2, 3, 5]].copy(), c=0.0)
    a, b = solve([pr], None, FIXED)[0], solve([pr], [zero], FIXED)[0]
    assert [r.iteration_status for r in a[0]] == [r.iteration_status for r in b[0]]
    assert [r.damping_term for r in a[0]] == [r.damping_term for r in b[0]]
    for x, y in zip(a[0], b[0]):
        assert abs(x.trial_cost - y.trial_cost) <= 1e-12 * abs(x.trial_cost)
        assert abs(x.cost - y.cost) <= 1e-12 * abs(x.cost)


def test_invalid_prior_is_refused_before_the_gpu(trio):
    from bundle_adjustment_solver_amd._lib import BaError
    probs, priors = trio
    b = BaBatch(probs)
    bad = dict(priors[0], poses=np.array([4, 2], np.int32))
    with pytest.raises(BaError, match="ascend"):
        b.set_prior([bad, None, None])
    with pytest.raises(BaError, match="fixed"):
        b.set_prior([dict(priors[0], poses=np.array([0, 4], np.int32)), None, None])
    assert b.prior_info()["n_prior"] == 0
    b.close()


# ---- 5. pinning ---------------------------------------------------------------------------------
def test_a_heavy_prior_pins_its_poses(built):
    """H = w I with w = 1e6 x the largest diagonal entry of A, b = 0, T_lin = the initial
    poses: the Hessian of a pinned pose is at least 1e6 times what it is without the prior
    while its gradient is the same, so it moves less than 1e-3 of its free motion."""
    pr = window(6, 29, True, 51)
    g = BaProblem(0)
    g.set_cameras(pr["cam_intr"], pr["cam_T"])
    g.set_poses(pr["pose_T"], pr["pose_fixed"])
    g.set_points(pr["pt_X"], pr["pt_fixed"])
    g.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
    g.finalize()
    g.stage_linearize(0.0, 1.0)
    A = g.get_A()[0].reshape(-1, 6, 6)
    g.close()
    w = 1e6 * max(np.diag(Aj).max() for Aj in A)
    poses = np.array([2, 4, 5], np.int32)
    pin = dict(poses=poses, H=w * np.eye(18), b=np.zeros(18), T_lin=pr["pose_T"][poses].copy(), c=0.0)
    kw = dict(max_iter=5, thr_step=0.0, thr_cost=0.0)
    free, held = solve([pr], None, kw)[0], solve([pr], [pin], kw)[0]
    for q in poses:
        moved_free = np.abs(free[2][q] - pr["pose_T"][q]).max()
        moved_held = np.abs(held[2][q] - pr["pose_T"][q]).max()
        print("pose %d: free %.3e pinned %.3e" % (q, moved_free, moved_held))
        assert moved_free > 0 and moved_held < 1e-3 * moved_free
    assert np.abs(held[2][3] - pr["pose_T"][3]).max() > 1e-3 * np.abs(free[2][3] - pr["pose_T"][3]).max()


# ---- 6. facade ----------------------------------------------------------------------------------
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


def _probs_of(solvers):
    out = []
    for sv in solvers:
        intr, camT, T_jw, X, pf, qf, ocam, opose, opt, ouv = sv._host_arrays()
        out.append(dict(cam_intr=intr, cam_T=camT, pose_T=T_jw, pose_fixed=pf, pt_X=X, pt_fixed=qf,
                        obs_cam=ocam, obs_pose=opose, obs_pt=opt, obs_uv=ouv))
    return out


def test_facade_priors_are_the_raw_call_in_scaled_units(built):
    sigma = 0.7
    scs = [scenes.ba_batch_scene(1, n_pose=6, n_pt=29, stereo=True, seed=61, n_fixed=2)[0],
           scenes.ba_batch_scene(1, n_pose=7, n_pt=31, stereo=False, seed=62, n_fixed=2)[0]]
    solvers = [_facade_solver(sc) for sc in scs]
    probs = _probs_of(solvers)
    raw = [prior_ref.random_prior(probs[0], [2, 3, 5], seed=7, c="constant"), None]
    Hu, bu = marginal_to_user_units(raw[0]["H"], raw[0]["b"], sigma)
    cu = raw[0]["c"] / (sigma ** 2 * 1e-4)
    lin = _T12_to_44(raw[0]["T_lin"])
    lin[:, :3, 3] *= 100.0
    user = [dict(poses=[2, 3, 5], H=Hu, b=bu, lin_poses=rigid_inverse(lin), c=cu), None]
    # what the facade hands to set_prior, and the raw call with exactly that
    sp = FullBundleAdjustmentSolver._scaled_priors("test", solvers, user, sigma)
    assert relerr(sp[0]["H"], raw[0]["H"]) < 1e-14 and relerr(sp[0]["T_lin"], raw[0]["T_lin"]) < 1e-14
    opts = Options()
    opts.iteration_handle.max_num_iterations = 5
    expect = solve(probs, sp, dict(max_iter=5, thr_step=opts.convergence_handle.threshold_step_size,
                                   thr_cost=opts.convergence_handle.threshold_cost_change,
                                   huber=opts.outlier_handle.threshold_huber_loss,
                                   lambda0=opts.trust_region_handle.initial_lambda,
                                   dec=opts.trust_region_handle.decrease_ratio_lambda,
                                   inc=opts.trust_region_handle.increase_ratio_lambda))
    res = FullBundleAdjustmentSolver.SolveBatch(solvers, opts, priors=user, sigma_pixel=sigma)
    after = _probs_of(solvers)
    for k in range(2):
        assert res[k].status == 0 and res[k].n_iter == expect[k][1].n_iter
        assert np.array_equal(after[k]["pose_T"], expect[k][2]) and np.array_equal(after[k]["pt_X"], expect[k][3])
    # and the other two entry points take the same keyword
    cov = FullBundleAdjustmentSolver.ComputeCovarianceBatch(solvers, sigma_pixel=sigma, priors=user)
    cov0 = FullBundleAdjustmentSolver.ComputeCovarianceBatch(solvers, sigma_pixel=sigma)
    assert not np.array_equal(cov[0][0], cov0[0][0]) and np.array_equal(cov[1][0], cov0[1][0])
    mg = FullBundleAdjustmentSolver.MarginalizeBatch(solvers, [[2], [2]], sigma_pixel=sigma, priors=user)
    mg0 = FullBundleAdjustmentSolver.MarginalizeBatch(solvers, [[2], [2]], sigma_pixel=sigma)
    assert not np.array_equal(mg[0][0], mg0[0][0]) and np.array_equal(mg[1][0], mg0[1][0])
