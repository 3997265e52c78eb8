"""GPU tests of the relative-pose factors of the batch path (ba_batch_set_relative as more
factors of ba_batch_solve, ba_batch_covariance and ba_batch_marginalize) against the host
references of rel_ref.

Tolerances are the project's, from test_gpu_batch_prior.py.  LM trajectories: identical
iteration_status, damping_term within 1e-12, cost and trial cost within 1e-7 relative, final
poses and points within 1e-6 relative.  Matrices: the two host routes must agree to 1e-8
(otherwise the scene is unfit), the GPU lies within 10 x max(noise, 1e-12)."""
import numpy as np
import pytest

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import BaError, make_options
from bundle_adjustment_solver_amd.solver import (BaBatch, FullBundleAdjustmentSolver, Options, _T12_to_44,
                                                 marginal_to_user_units, relative_residual, rigid_inverse)
from oracle import oracle_py as O

import cov_ref
import marg_ref
import prior_ref
import rel_cases
import rel_ref
from rel_cases import FIXED, window
from test_gpu_batch_prior import (_facade_solver, _probs_of, assert_same_bits, check_trajectory, relerr)

pytestmark = pytest.mark.gpu


def solve(probs, rels, opt_kw, priors=None, calls=1):
    """-> per problem (rows, result, poses, points) of a fresh batch; calls > 1 re-solves the
    same start values and requires the bits of the first call"""
    b = BaBatch(probs)
    if rels is not None:
        b.set_relative(rels)
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


# ---- 3. LM trajectory parity ------------------------------------------------------------------
@pytest.fixture(scope="module")
def parity(built):
    cases = rel_cases.parity_cases()
    ref = [rel_ref.lm_with_relatives(pr, rels, O.make_options(**FIXED)) for _, _, pr, rels in cases]
    got = solve([c[2] for c in cases], [c[3] for c in cases], FIXED)
    return cases, ref, got


def test_lm_trajectory_matches_the_reference_loop(parity):
    cases, ref, got = parity
    for k, (name, _, pr, rels) in enumerate(cases):
        st = {r.iteration_status for r in ref[k][0]}
        assert 2 in st and (0 in st or 1 in st), (name, st)
        check_trajectory(name, got[k], ref[k])
    # the factors are felt: without them the first trial cost differs by far more than the tolerance
    free = solve([c[2] for c in cases], None, FIXED)
    for k in range(len(cases)):
        assert relerr(free[k][0][0].trial_cost, got[k][0][0].trial_cost) > 1e-4


def test_gauss_newton_matches_the_reference_loop(built):
    kw = dict(max_iter=4, thr_step=0.0, thr_cost=0.0, gauss_newton=True, lambda0=1e-3)
    for name, _, pr, rels in rel_cases.parity_cases():
        ref = rel_ref.lm_with_relatives(pr, rels, O.make_options(**kw))
        check_trajectory("gauss-newton " + name, solve([pr], [rels], kw)[0], ref)


# ---- 4. equivalence with the prior --------------------------------------------------------------
@pytest.mark.parametrize("j,k", [(3, 1), (4, 0)])
def test_single_factor_to_a_fixed_pose_is_the_prior(built, j, k):
    """(j optimisable, k fixed, Z, Omega) is the prior on pose j with H = Omega, b = 0, c = 0,
    T_lin = Z T_k: the same residual, Jacobian (identity), cost term and damping."""
    pr = window(6, 29, True, 31)
    assert pr["pose_fixed"][k] and not pr["pose_fixed"][j]
    rels = rel_ref.random_relatives(pr, [(j, k)], seed=8, strength=30.0)
    T_lin = prior_ref.compose(rels["Z"][0], pr["pose_T"][k])
    prior = dict(poses=np.array([j], np.int32), H=rels["Omega"][0].copy(), b=np.zeros(6), T_lin=T_lin[None, :], c=0.0)
    as_rel = solve([pr], [rels], FIXED)[0]
    as_prior = solve([pr], None, FIXED, priors=[prior])[0]
    ref = prior_ref.lm_with_prior(pr, prior, O.make_options(**FIXED))
    check_trajectory("factor", as_rel, ref)
    check_trajectory("prior", as_prior, ref)
    check_trajectory("factor against prior", as_rel, (as_prior[0], None, as_prior[2], as_prior[3]))
    free = solve([pr], None, FIXED)[0]
    assert relerr(free[0][0].trial_cost, as_rel[0][0].trial_cost) > 1e-4


# ---- 5. more factors than threads ---------------------------------------------------------------
def test_more_factors_than_threads(built):
    """16 optimisable poses, every pair coupled three times in both orientations: 360 factors
    against 256 threads, 120 coupled blocks of three factors each"""
    pr = window(18, 45, True, 33)
    opt = np.flatnonzero(pr["pose_fixed"] == 0)
    assert len(opt) == 16
    pairs = []
    for rep in range(3):
        for a in range(16):
            for b in range(a):
                pairs.append((opt[a], opt[b]) if (a + b + rep) % 2 else (opt[b], opt[a]))
    assert len(pairs) == 360
    rels = rel_ref.random_relatives(pr, pairs, seed=12, strength=0.02)
    ref = rel_ref.lm_with_relatives(pr, rels, O.make_options(**FIXED))
    filler = window(6, 29, True, 41)
    frels = rel_ref.random_relatives(filler, rel_cases.chain(6), seed=13)
    alone = solve([pr], [rels], FIXED, calls=2)
    check_trajectory("360 factors", alone[0], ref)
    free = solve([pr], None, FIXED)[0]
    assert relerr(free[0][0].trial_cost, alone[0][0][0].trial_cost) > 1e-4
    moved = solve([filler, filler, pr, filler], [frels, None, rels, frels], FIXED)
    assert_same_bits(alone, [moved[2]])
    b = BaBatch([filler, pr])
    b.set_relative([frels, rels])
    info = b.relative_info()
    b.close()
    assert info["n_problems"] == 2 and info["n_factors"] == 364 and info["device_bytes"] >= 364 * 126 * 8


# ---- 6. marginalisation and covariance ----------------------------------------------------------
# name -> (image columns, pairs): factors on marked, kept and fixed poses; pairs of two unmarked
# poses do not join, among them the only factor of the far pose
MARG = {
    "mono8_m2": (64, [(3, 2), (4, 3), (2, 1), (0, 3), (6, 2), (3, 2), (5, 4), (7, 6), (1, 4)]),
    "stereo18_m1": (112, [(3, 2), (2, 1), (10, 2), (0, 2), (2, 9), (5, 4), (17, 16), (12, 1)]),
}


@pytest.mark.parametrize("name", sorted(MARG))
def test_marginalize_and_covariance_with_factors(built, name):
    cols, pairs = MARG[name]
    pr, mk, far = marg_ref.build_scene(name)
    assert marg_ref.image_columns(pr, mk) == cols
    rels = rel_ref.random_relatives(pr, pairs, seed=14)
    rH, rb, noise, rkept, _, flags = rel_ref.marg_with_relatives(pr, mk, rels)
    fH, fb, _, _, _ = marg_ref.reference(pr, mk)
    rp, rq, cnoise = rel_ref.cov_with_relatives(pr, rels)
    fp, _, _ = prior_ref.cov_with_prior(pr, None)
    assert flags.any() and not flags.all()
    b = BaBatch([pr])
    b.set_relative([rels])
    Hl, bl, kl, res = b.marginalize(mk, 1.0)
    plan = b.relative_marg_plan(mk)
    cp, cq, cres = b.covariance(1.0)
    b.close()
    eH, eb = marg_ref.rel_diff(Hl[0], rH), marg_ref.rel_diff(bl[0], rb)
    ep, eq = cov_ref.rel_block_diff(cp, rp), cov_ref.rel_block_diff(cq, rq)
    print("%s: marg noise %.3e gpu H %.3e b %.3e | cov noise %.3e gpu pose %.3e point %.3e"
          % (name, noise, eH, eb, cnoise, ep, eq))
    assert noise <= 1e-8 and cnoise <= 1e-8, "scene unfit: the two host references disagree"
    assert res[0].status == 0 and res[0].dropped_pivots == 0 and np.array_equal(kl[0], rkept)
    assert cres[0].status == 0 and cres[0].dropped_pivots == 0
    assert np.array_equal(plan, flags)
    tol = 10.0 * max(noise, 1e-12)
    assert eH <= tol and eb <= tol, (eH, eb, tol)
    ctol = 10.0 * max(cnoise, 1e-12)
    assert ep <= ctol and eq <= ctol, (ep, eq, ctol)
    assert np.array_equal(Hl[0], Hl[0].T)
    # the factors are in the results
    assert marg_ref.rel_diff(Hl[0], fH) > 1e-6 and marg_ref.rel_diff(bl[0], fb) > 1e-6
    assert cov_ref.rel_block_diff(cp, fp) > 1e-6
    # the far pose touches neither L nor a joining factor: exactly zero rows and columns; a
    # kept pose that a joining factor touches has non-zero ones
    kept = list(kl[0])
    at = lambda q: slice(6 * kept.index(q), 6 * kept.index(q) + 6)
    assert not Hl[0][at(far), :].any() and not Hl[0][:, at(far)].any() and not bl[0][at(far)].any()
    touched = [int(q) for f, (j, k) in enumerate(pairs) if flags[f] for q in (j, k) if q in kept]
    assert touched
    for q in touched:
        assert Hl[0][at(q), at(q)].any()


def test_a_marked_fixed_pose_takes_its_factors_along(built):
    """'optimisable or fixed': mono8_m2 with the fixed pose 1 marked as well.  It owns no columns
    but leaves the window, so the factors (1, 4) and (5, 1), whose other pose is kept and
    unmarked, join as unary factors on poses 4 and 5 (and its landmarks join L)."""
    pairs = MARG["mono8_m2"][1] + [(5, 1)]
    pr, mk, _ = marg_ref.build_scene("mono8_m2")
    assert pr["pose_fixed"][1] and not mk[1]
    mk = mk.copy()
    mk[1] = 1
    rels = rel_ref.random_relatives(pr, pairs, seed=14)
    rH, rb, noise, rkept, _, flags = rel_ref.marg_with_relatives(pr, mk, rels)
    only = [f for f, (j, k) in enumerate(pairs) if 1 in (j, k) and not (mk[j] and mk[k])]
    assert [pairs[f] for f in only] == [(1, 4), (5, 1)] and flags[only].all()
    # the same without the rule: those two factors left out
    off = flags.copy()
    off[only] = 0
    T = np.asarray(pr["pose_T"], np.float64)
    dH = rel_ref.dense_factors(pr, T, rels, flags)[0] - rel_ref.dense_factors(pr, T, rels, off)[0]
    b = BaBatch([pr])
    b.set_relative([rels])
    Hl, bl, kl, res = b.marginalize(mk, 1.0)
    plan = b.relative_marg_plan(mk)
    H0 = b.marginalize(mk * (np.arange(len(mk)) != 1), 1.0)[0]
    b.close()
    eH, eb = marg_ref.rel_diff(Hl[0], rH), marg_ref.rel_diff(bl[0], rb)
    print("fixed pose marked: marg noise %.3e gpu H %.3e b %.3e" % (noise, eH, eb))
    assert noise <= 1e-8, "scene unfit: the two host references disagree"
    assert res[0].status == 0 and res[0].dropped_pivots == 0 and np.array_equal(kl[0], rkept)
    assert np.array_equal(plan, flags)
    tol = 10.0 * max(noise, 1e-12)
    assert eH <= tol and eb <= tol, (eH, eb, tol)
    # the two factors weigh in: their blocks are far above the tolerance, and marking the fixed
    # pose changed the result
    assert np.abs(dH).max() > 1e-6 * np.abs(rH).max()
    assert marg_ref.rel_diff(Hl[0], H0[0]) > 1e-6


# ---- 7. slide consistency -----------------------------------------------------------------------
GN1 = dict(max_iter=1, thr_step=0.0, thr_cost=0.0, gauss_newton=True, lambda0=0.0)


def slide(pr, mk, rels):
    """one GN step of the full window with all factors, and of the reduced window with the
    factors that did not leave plus the marginal as its prior: (kept poses and surviving
    points of both, the kept poses before the step)"""
    full = BaBatch([pr])
    full.set_relative([rels])
    Hl, bl, kl, res = full.marginalize(mk, 1.0)
    leaves = full.relative_marg_plan(mk)
    assert res[0].status == 0 and res[0].dropped_pivots == 0
    sub, kp, keep_p, keep_q = prior_ref.reduced_window(pr, mk)
    assert np.array_equal(keep_p[kp], kl[0])
    prior = dict(poses=kp, H=Hl[0].copy(), b=bl[0].copy(), T_lin=sub["pose_T"][kp].copy(), c=0.0)
    stay = rel_ref.subset(rels, leaves == 0)
    stay["j"] = np.searchsorted(keep_p, stay["j"]).astype(np.int32)
    stay["k"] = np.searchsorted(keep_p, stay["k"]).astype(np.int32)
    assert leaves.any() and rel_ref.n_factors(stay) > 0
    full.solve(make_options(**GN1))
    Tf, Xf = full.get_poses()[keep_p], full.get_points()[keep_q]
    full.close()
    Tr, Xr = solve([sub], [stay], GN1, priors=[prior])[0][2:]
    return (Tf, Xf), (Tr, Xr), sub["pose_T"]


@pytest.mark.parametrize("name", ["mono5_m1", "stereo4_m1"])
def test_slide_consistency(built, name):
    pr, mk, _ = marg_ref.build_scene(name)
    n = len(pr["pose_fixed"])
    first = int(np.flatnonzero(pr["pose_fixed"] == 0)[0])
    assert mk[first] and mk.sum() == 1          # the oldest optimisable pose leaves
    rels = rel_ref.random_relatives(pr, rel_cases.chain(n, first - 1), seed=15)
    # Converged in Gauss-Newton mode: with measurements that the window cannot meet (r != 0 at
    # the optimum) the LM controller, which judges a step by the sum of residual NORMS, stalls
    # short of the least-squares optimum the linearisation aims at (seen on the CPU in the
    # reference loop: 16 LM iterations leave a Gauss-Newton step of 2e-2 in the mono window).
    # 48 iterations: the stereo window converges linearly, by 0.87 per iteration (its cross
    # blocks follow the last-writer rule), to 4e-4 of the first step.
    conv = solve([pr], [rels], dict(max_iter=48, thr_step=0.0, thr_cost=0.0, gauss_newton=True, lambda0=1e-6))[0]
    pr_conv = dict(pr, pose_T=conv[2], pt_X=conv[3])
    steps = {}
    for label, p in (("perturbed", pr), ("converged", pr_conv)):
        (Tf, Xf), (Tr, Xr), T0 = slide(p, mk, rels)
        print("%s %s: reduced against full window: poses %.3e points %.3e"
              % (name, label, marg_ref.rel_diff(Tr, Tf), marg_ref.rel_diff(Xr, Xf)))
        steps[label] = (np.abs(Tr - T0).max(), np.abs(Tf - T0).max())
    print("%s: steps (reduced, full) %s" % (name, steps))
    assert steps["perturbed"][0] > 0
    assert steps["converged"][0] < 1e-2 * steps["perturbed"][0]


# ---- 8. bits ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trio(built):
    probs = [window(6, 29, True, 41), window(7, 31, False, 42), window(5, 27, True, 43)]
    rels = [rel_ref.random_relatives(probs[0], rel_cases.chain(6) + [(5, 2)], seed=1), None,
            rel_ref.random_relatives(probs[2], [(2, 0), (4, 3), (3, 4)], seed=2)]
    return probs, rels


def test_set_then_clear_is_the_never_set_batch(trio):
    probs, rels = trio
    never = solve(probs, None, FIXED)
    b = BaBatch(probs)
    b.set_relative(rels)
    info = b.relative_info()
    assert info["n_problems"] == 2 and info["n_factors"] == 8 and info["device_bytes"] > 0
    b.clear_relative()
    assert b.relative_info() == dict(n_problems=0, n_factors=0, device_bytes=0)
    rows, res = b.solve(make_options(**FIXED))
    T, X = b.get_poses(), b.get_points()
    b.close()
    got = [(rows[p], res[p], b.poses_of(p, T), b.points_of(p, X)) for p in range(3)]
    assert_same_bits(never, got)


def test_problem_without_factors_between_two_with(trio):
    probs, rels = trio
    got = solve(probs, rels, FIXED)
    assert_same_bits([got[1]], solve([probs[1]], None, FIXED))
    # and so for the other two kernels
    b, alone = BaBatch(probs), BaBatch([probs[1]])
    b.set_relative(rels)
    mk = np.zeros(b.n_pose, np.uint8)
    mk[b.pose_off[:-1] + 2] = 1
    Hl, bl, _, _ = b.marginalize(mk, 1.0)
    H1, b1, _, _ = alone.marginalize(mk[b.pose_off[1]:b.pose_off[2]], 1.0)
    assert np.array_equal(Hl[1], H1[0]) and np.array_equal(bl[1], b1[0])
    cp, cq, _ = b.covariance(1.0)
    cp1, cq1, _ = alone.covariance(1.0)
    assert np.array_equal(b.cov_poses_of(1, cp), cp1) and np.array_equal(b.cov_points_of(1, cq), cq1)
    b.close()
    alone.close()


def test_position_independence_and_repeats(trio):
    probs, rels = trio
    alone = solve([probs[0]], [rels[0]], FIXED, calls=3)
    filler, fr = [probs[1], probs[2], probs[1], probs[2]], [None, rels[2], None, None]
    first = solve([probs[0]] + filler, [rels[0]] + fr, FIXED)
    last = solve(filler + [probs[0]], fr + [rels[0]], FIXED)
    assert_same_bits(alone, [first[0]])
    assert_same_bits(alone, [last[4]])
    assert not np.array_equal(alone[0][2], solve([probs[0]], None, FIXED)[0][2])


def test_factors_on_a_problem_over_the_limit_are_ignored(trio):
    probs, rels = trio
    big = window(20, 30, False, 44, n_fixed=2)            # 18 optimisable poses: status 2
    rb = rel_ref.random_relatives(big, [(3, 2), (2, 1)], seed=3)
    got = solve([probs[0], big, probs[2]], [rels[0], rb, rels[2]], FIXED)
    assert got[1][1].status == 2 and np.array_equal(got[1][2], big["pose_T"])
    ref = solve([probs[0], probs[2]], [rels[0], rels[2]], FIXED)
    assert_same_bits(ref, [got[0], got[2]])
    b = BaBatch([probs[0], big, probs[2]])
    b.set_relative([rels[0], rb, rels[2]])
    assert b.relative_info()["n_factors"] == 8
    mk = np.zeros(b.n_pose, np.uint8)
    mk[b.pose_off[:-1] + 2] = 1
    plan = b.relative_marg_plan(mk)
    b.close()
    assert len(plan) == 10 and not plan[5:7].any() and plan[:5].any()


def test_factors_survive_update_values(trio):
    probs, rels = trio
    want = solve(probs, rels, FIXED)
    b = BaBatch(probs)
    b.set_relative(rels)
    T0, X0 = b.get_poses(), b.get_points()
    b.solve(make_options(**FIXED))
    b.update_values(T0, X0)
    assert b.relative_info()["n_factors"] == 8
    rows, res = b.solve(make_options(**FIXED))
    T, X = b.get_poses(), b.get_points()
    b.close()
    assert_same_bits(want, [(rows[p], res[p], b.poses_of(p, T), b.points_of(p, X)) for p in range(3)])


def test_invalid_factors_are_refused_and_change_nothing(trio):
    probs, rels = trio
    b = BaBatch(probs)
    b.set_relative(rels)
    with pytest.raises(BaError, match="problem 0, factor 1"):
        b.set_relative([dict(rels[0], k=np.array([1, 3, 3, 4, 2], np.int32)), None, None])   # j == k == 3
    with pytest.raises(BaError, match="both poses are fixed"):
        b.set_relative([None, None, dict(rels[2], j=np.array([1, 4, 3], np.int32))])
    assert b.relative_info()["n_factors"] == 8
    b.close()


# ---- 9. pinning -----------------------------------------------------------------------------------
def test_a_heavy_factor_pins_its_relative_pose(built):
    """Omega = w I with w = 1e6 x the largest entry of A: the pair's relative pose follows the
    measurement while the pair as a whole still moves with the reprojections.  Gauss-Newton
    mode: the LM gain ratio divides a difference of residual NORMS (which grow like sqrt(w))
    by the quadratic model (which grows like w), so with this weight it is 1e-2 for a perfect
    step and the controller rejects every step (seen on the CPU in the reference loop); the
    Gauss-Newton mode takes them."""
    pr = window(6, 29, True, 51)
    j, k = 4, 2
    w = 1e6 * rel_ref.a_scale(pr) ** 2
    rels = rel_ref.random_relatives(pr, [(j, k)], seed=16)
    rels["Omega"] = w * np.eye(6)[None]
    kw = dict(max_iter=5, thr_step=0.0, thr_cost=0.0, gauss_newton=True, lambda0=1e-3)
    free, held = solve([pr], None, kw)[0], solve([pr], [rels], kw)[0]
    norm = lambda T: np.sqrt(np.sum(relative_residual(T[j], T[k], rels["Z"][0]) ** 2))
    r_free, r_held = norm(free[2]), norm(held[2])
    print("|r| free %.3e pinned %.3e (start %.3e)" % (r_free, r_held, norm(pr["pose_T"])))
    assert r_free > 1e-4 and r_held < 1e-3 * r_free
    for q in (j, k):
        moved_free = np.abs(free[2][q] - pr["pose_T"][q]).max()
        moved_held = np.abs(held[2][q] - pr["pose_T"][q]).max()
        print("pose %d: free %.3e pinned pair %.3e" % (q, moved_free, moved_held))
        assert moved_held > 1e-1 * moved_free


# ---- 10. facade -----------------------------------------------------------------------------------
def test_facade_relatives_are_the_raw_call_in_scaled_units(built):
    sigma = 0.7
    scs = [scenes.ba_batch_scene(1, n_pose=6, n_pt=29, stereo=True, seed=61, n_fixed=2)[0],
           scenes.ba_batch_scene(1, n_pose=7, n_pt=31, stereo=False, seed=62, n_fixed=2)[0]]
    solvers = [_facade_solver(sc) for sc in scs]
    probs = _probs_of(solvers)
    raw = [rel_ref.random_relatives(probs[0], [(3, 2), (2, 1), (0, 5), (3, 2)], seed=7), None]
    # the same factors in the caller's units: the measurement pose_j^-1 pose_k of AddPose's
    # poses (T_jw T_kw^-1 after its conversion, translation in user units), Omega by the rule
    # of marginal_to_user_units for a 6x6 H
    Zu = _T12_to_44(raw[0]["Z"])
    Zu[:, :3, 3] *= 100.0
    user = [[dict(pose_j=j, pose_k=k, measurement=Zu[f],
                  information=marginal_to_user_units(raw[0]["Omega"][f], np.zeros(6), sigma)[0])
             for f, (j, k) in enumerate(zip(raw[0]["j"], raw[0]["k"]))], None]
    sr = FullBundleAdjustmentSolver._scaled_relatives("test", solvers, user, sigma)
    assert sr[1] is None and np.array_equal(sr[0]["j"], raw[0]["j"]) and np.array_equal(sr[0]["k"], raw[0]["k"])
    assert relerr(sr[0]["Omega"], raw[0]["Omega"]) < 1e-14 and relerr(sr[0]["Z"], raw[0]["Z"]) < 1e-14
    opts = Options()
    opts.iteration_handle.max_num_iterations = 5
    expect = solve(probs, sr, dict(max_iter=5, thr_step=opts.convergence_handle.threshold_step_size,
                                   thr_cost=opts.convergence_handle.threshold_cost_change,
                                   huber=opts.outlier_handle.threshold_huber_loss,
                                   lambda0=opts.trust_region_handle.initial_lambda,
                                   dec=opts.trust_region_handle.decrease_ratio_lambda,
                                   inc=opts.trust_region_handle.increase_ratio_lambda))
    cov0 = FullBundleAdjustmentSolver.ComputeCovarianceBatch(solvers, sigma_pixel=sigma)
    mg0 = FullBundleAdjustmentSolver.MarginalizeBatch(solvers, [[2], [2]], sigma_pixel=sigma)
    cov = FullBundleAdjustmentSolver.ComputeCovarianceBatch(solvers, sigma_pixel=sigma, relatives=user)
    mg = FullBundleAdjustmentSolver.MarginalizeBatch(solvers, [[2], [2]], sigma_pixel=sigma, relatives=user)
    assert not np.array_equal(cov[0][0], cov0[0][0]) and np.array_equal(cov[1][0], cov0[1][0])
    assert not np.array_equal(mg[0][0], mg0[0][0]) and np.array_equal(mg[1][0], mg0[1][0])
    # which factors left with pose 2: everything that names it
    assert list(mg[0][-1]) == [1, 1, 0, 1] and len(mg[1][-1]) == 0
    res = FullBundleAdjustmentSolver.SolveBatch(solvers, opts, relatives=user, sigma_pixel=sigma)
    after = _probs_of(solvers)
    for k in range(2):
        assert res[k].status == 0 and res[k].n_iter == expect[k][1].n_iter
        assert np.array_equal(after[k]["pose_T"], expect[k][2]) and np.array_equal(after[k]["pt_X"], expect[k][3])
