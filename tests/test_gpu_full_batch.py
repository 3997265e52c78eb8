"""GPU tests of the batched full bundle adjustment (ba_batch_*: one persistent
workgroup per problem, the whole LM loop in one launch) against the CPU oracle and
the handle path (BaProblem.solve), with the project's tolerances: identical
iteration_status per row, damping_term within 1e-12, cost and trial cost within 1e-7
relative, final poses and points within 1e-6 relative.  Parity runs use thr_step =
thr_cost = 0 and a fixed iteration count, so the stop rule cannot desynchronise the
two sides."""
import copy

import numpy as np
import pytest

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import (BaBatch, BaProblem, Camera,
                                                 FullBundleAdjustmentSolver, Options,
                                                 Summary)
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu
ITERS = 6
FIXED = dict(max_iter=ITERS, thr_step=0.0, thr_cost=0.0)
ROW_FIELDS = ("cost", "cost_change", "average_reprojection_error", "abs_gradient", "abs_step",
              "damping_term", "iteration_status", "rho", "model_change", "trial_cost")


def relerr(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def row_bits(rows):
    """every deterministic field of the rows (iter_time_ms is a clock reading)"""
    return np.array([[getattr(r, f) for f in ROW_FIELDS] for r in rows], float).reshape(-1, len(ROW_FIELDS))


def make_gpu(pr):
    p = BaProblem(0)
    p.set_cameras(pr["cam_intr"], pr["cam_T"])
    p.set_poses(pr["pose_T"], pr["pose_fixed"])
    p.set_points(pr["pt_X"], pr["pt_fixed"])
    p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
    p.finalize()
    return p


def assert_same_trajectory(rows, orows, rtol_cost=1e-7):
    assert len(rows) == len(orows)
    floor = 1e-12 * abs(orows[0].cost)
    for k, (a, b) in enumerate(zip(rows, orows)):
        assert a.iteration_status == b.iteration_status, k
        assert relerr(a.damping_term, b.damping_term) < 1e-12, k
        assert abs(a.trial_cost - b.trial_cost) <= rtol_cost * abs(b.trial_cost) + floor, k
        assert abs(a.cost - b.cost) <= rtol_cost * abs(b.cost) + floor, k


def window(n_pose, n_pt, stereo, seed, n_fixed=2, **kw):
    return scenes.ba_batch_scene(1, n_pose=n_pose, n_pt=n_pt, stereo=stereo, seed=seed,
                                 n_fixed=n_fixed, **kw)[0]


def five_problems():
    """The parity batch: different shapes, every one compared.
      0  stereo window of the reference scene (test_ba_scene): its last 10 poses, 2 fixed,
         the 80 landmarks seen only there — and the scene's 130 landmarks nobody sees
         (zero C_i: Cinv_i = 0, they stay where they are)
      1  mono window, 5 poses / 37 landmarks
      2  one free pose (3 of 4 fixed)
      3  exactly 16 free poses (18 poses, 2 fixed): the full 96-column image
      4  landmarks seen by fixed poses only, and some fixed points"""
    out = [scenes.pose_window_subscene(scenes.test_ba_scene(), 50, 60, n_fixed=2),
           window(5, 37, False, 11),
           window(4, 29, True, 12, n_fixed=3),
           window(18, 45, True, 13),
           window(7, 41, True, 14, n_fixed=3)]
    sc = out[4]
    lone = np.arange(0, 41, 5)                 # these landmarks keep only fixed-pose observations
    keep = ~(np.isin(sc["obs_pt"], lone) & (sc["obs_pose"] >= 3))
    for k in ("obs_cam", "obs_pose", "obs_pt", "obs_uv"):
        sc[k] = sc[k][keep]
    sc["pt_fixed"] = sc["pt_fixed"].copy()
    sc["pt_fixed"][[2, 17, 33]] = True
    sc["X_init"] = sc["X_init"].copy()
    sc["X_init"][[2, 17, 33]] = sc["X_true"][[2, 17, 33]]
    return [scenes.scaled_problem(s) for s in out]


class Ref:
    """oracle and handle-path results of a problem list, computed once"""

    def __init__(self, probs, opt_kw):
        self.probs = probs
        self.oracle, self.handle = [], []
        for pr in probs:
            o = O.Oracle(pr)
            orows, oconv = o.solve(O.make_options(**opt_kw))
            self.oracle.append((orows, oconv, o.get_poses(), o.get_points()))
            g = make_gpu(pr)
            rows, conv = g.solve(make_options(**opt_kw))
            self.handle.append((rows, conv, g.get_poses(), g.get_points()[0],
                                g.get_dropped_pivots()))
            g.close()


def solve_batch(probs, opt_kw, cap=None):
    b = BaBatch(probs)
    rows, res = b.solve(make_options(**opt_kw), cap)
    T, X = b.get_poses(), b.get_points()
    out = [(rows[p], res[p], b.poses_of(p, T).copy(), b.points_of(p, X).copy())
           for p in range(len(probs))]
    b.close()
    return out


@pytest.fixture(scope="module")
def five(built):
    probs = five_problems()
    assert [int((p["pose_fixed"] == 0).sum()) for p in probs] == [8, 3, 1, 16, 4]
    assert np.bincount(probs[0]["obs_pt"], minlength=len(probs[0]["pt_X"])).tolist().count(0) == 130
    assert all(p["obs_pt"].size > 0 for p in probs)
    return probs, Ref(probs, FIXED), solve_batch(probs, FIXED)


def check_against(got, orows, oT, oX):
    rows, res, T, X = got
    assert res.status == 0 and res.n_iter == len(orows) == res.n_rows
    assert_same_trajectory(rows, orows)
    assert relerr(T, oT) < 1e-6 and relerr(X, oX) < 1e-6


def test_parity_with_oracle_and_handle_path(five):
    probs, ref, got = five
    for p in range(len(probs)):
        orows, _, oT, oX = ref.oracle[p]
        check_against(got[p], orows, oT, oX)
        hrows, _, hT, hX, _ = ref.handle[p]
        check_against(got[p], hrows, hT, hX)
        assert got[p][1].dropped_pivots == 0
    # the fixed members of problem 4 did not move, its lone landmarks did
    pr = probs[4]
    assert np.array_equal(got[4][2][:3], pr["pose_T"][:3])
    assert np.array_equal(got[4][3][[2, 17, 33]], pr["pt_X"][[2, 17, 33]])
    assert not np.array_equal(got[4][3][[0, 5]], pr["pt_X"][[0, 5]])


def test_isolation_and_determinism(five):
    probs, _, got = five
    again = solve_batch(probs, FIXED)
    rev = solve_batch(probs[::-1], FIXED)[::-1]
    for p in range(len(probs)):
        alone = solve_batch([probs[p]], FIXED)[0]
        for other in (alone, again[p], rev[p]):
            assert np.array_equal(got[p][2], other[2]) and np.array_equal(got[p][3], other[3])
            assert np.array_equal(row_bits(got[p][0]), row_bits(other[0]))


def quirk_problems():
    """0: stereo, both cameras see every (landmark, pose) pair -> the last-writer rule
    decides every cross block (and the observation order is shuffled inside landmarks,
    so that the writer is not always the right camera); 1: pixel noise sigma = 0.5 px
    with Huber 1.0 px: the robust branch is active."""
    a = window(6, 33, True, 21)
    rng = np.random.default_rng(5)
    perm = rng.permutation(a["obs_pt"].size)
    for k in ("obs_cam", "obs_pose", "obs_pt", "obs_uv"):
        a[k] = a[k][perm]
    b = window(6, 33, True, 22, pixel_sigma=0.5)
    return [scenes.scaled_problem(a), scenes.scaled_problem(b)]


def test_last_writer_and_huber_quirks(built):
    probs = quirk_problems()
    pr = probs[0]
    key = pr["obs_pt"].astype(np.int64) * 64 + pr["obs_pose"]
    assert np.unique(key).size * 2 == key.size           # every pair observed twice
    last_cam = {k: c for k, c in zip(key, pr["obs_cam"])}
    assert 0 < sum(last_cam.values()) < len(last_cam)      # both cameras win somewhere
    ref = Ref(probs, FIXED)
    got = solve_batch(probs, FIXED)
    for p in range(2):
        check_against(got[p], *[ref.oracle[p][k] for k in (0, 2, 3)])
        check_against(got[p], *[ref.handle[p][k] for k in (0, 2, 3)])
    # In the solver's scaled units (0.01 px) a threshold of 1.0 is 100 px: it weights
    # nothing here.  0.005 (0.5 px) weights most observations of the noisy problem from
    # the first iteration on: the robust branch proper, checked the same way.
    hub = dict(FIXED, huber=0.005)
    rh = Ref(probs[1:], hub)
    gh = solve_batch(probs[1:], hub)[0]
    check_against(gh, *[rh.oracle[0][k] for k in (0, 2, 3)])
    check_against(gh, *[rh.handle[0][k] for k in (0, 2, 3)])
    assert relerr(gh[0][0].trial_cost, got[1][0][0].trial_cost) > 1e-4


def test_nan_cost_branch_and_skipped_steps(built):
    """One NaN pixel makes every cost NaN: rho = NaN fails every comparison of the
    control step (reference :939-953), so each step is SKIPPED, lambda stays,
    previous_cost advances to the NaN trial cost and the parameters never move.  After a
    SKIPPED step the kernel keeps its blocks and only damps again; the rows must be the
    oracle's."""
    pr = copy.deepcopy(quirk_problems()[0])
    pr["obs_uv"][123, 0] = np.nan
    kw = dict(max_iter=4, thr_step=-1.0, thr_cost=-1.0)
    orows, oconv = O.Oracle(pr).solve(O.make_options(**kw))
    rows, res, T, X = solve_batch([pr], kw)[0]
    assert res.status == 0 and res.n_iter == len(orows) == 4 and bool(res.converged) == oconv
    for a, b in zip(rows, orows):
        assert a.iteration_status == b.iteration_status == 2
        assert a.damping_term == b.damping_term == 100.0
        assert np.isnan(a.trial_cost) and np.isnan(b.trial_cost) and np.isnan(a.rho)
        assert np.isnan(a.cost) == np.isnan(b.cost)
    assert np.array_equal(T, pr["pose_T"]) and np.array_equal(X, pr["pt_X"])


def test_gauss_newton(built):
    pr = scenes.scaled_problem(window(5, 31, True, 23, pose_noise=0.01, point_noise=0.02))
    kw = dict(FIXED, gauss_newton=True, lambda0=1e-3)
    orows, _ = (o := O.Oracle(pr)).solve(O.make_options(**kw))
    got = solve_batch([pr], kw)[0]
    assert all(r.iteration_status == 0 and r.damping_term == orows[0].damping_term for r in got[0])
    check_against(got, orows, o.get_poses(), o.get_points())


def test_limits_and_bad_members(five):
    probs, ref, got = five
    big = scenes.scaled_problem(window(19, 30, False, 31))        # 17 free poses
    assert int((big["pose_fixed"] == 0).sum()) == 17
    mixed = solve_batch([probs[1], big, probs[2]], FIXED)
    assert mixed[1][1].status == 2 and mixed[1][1].n_iter == 0 and mixed[1][1].n_rows == 0
    assert np.array_equal(mixed[1][2], big["pose_T"]) and np.array_equal(mixed[1][3], big["pt_X"])
    without = solve_batch([probs[1], probs[2]], FIXED)
    for a, b in ((mixed[0], without[0]), (mixed[2], without[1])):
        assert a[1].status == 0
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        assert np.array_equal(row_bits(a[0]), row_bits(b[0]))
    # more than 64 poses in all is a limit too (60 further fixed poses nobody observes)
    many = copy.deepcopy(probs[1])
    many["pose_T"] = np.concatenate([many["pose_T"], np.repeat(many["pose_T"][:1], 60, axis=0)])
    many["pose_fixed"] = np.concatenate([many["pose_fixed"], np.ones(60, np.uint8)])
    assert solve_batch([many], FIXED)[0][1].status == 2
    many["pose_T"], many["pose_fixed"] = many["pose_T"][:64], many["pose_fixed"][:64]
    ok64 = solve_batch([many], FIXED)[0]
    assert ok64[1].status == 0 and np.array_equal(ok64[2][:5], without[0][2])


def test_dropped_pivots_nan_input_and_zero_iterations(five):
    probs, ref, _ = five
    # a free pose without observations: its six pivots are dropped in every factorisation
    lonely = copy.deepcopy(probs[1])
    keep = lonely["obs_pose"] != 4
    for k in ("obs_cam", "obs_pose", "obs_pt", "obs_uv"):
        lonely[k] = lonely[k][keep]
    r = Ref([lonely], FIXED)
    nanp = copy.deepcopy(probs[2])
    nanp["pt_X"][7, 1] = np.nan
    got = solve_batch([lonely, nanp, probs[0]], FIXED)
    assert got[0][1].status == 0
    assert got[0][1].dropped_pivots == r.handle[0][4] > 0
    check_against(got[0], *[r.handle[0][k] for k in (0, 2, 3)])
    assert np.array_equal(got[0][2][4], lonely["pose_T"][4])
    assert got[1][1].status == 1 and got[1][1].n_iter == 0
    assert np.array_equal(got[1][2], nanp["pose_T"])
    assert np.array_equal(got[1][3], nanp["pt_X"], equal_nan=True)
    check_against(got[2], *[ref.oracle[0][k] for k in (0, 2, 3)])
    zero = solve_batch(probs[:2], dict(FIXED, max_iter=0))
    for p in range(2):
        rows, res, T, X = zero[p]
        assert rows == [] and res.n_iter == 0 and res.converged == 1 and res.status == 0
        assert np.array_equal(T, probs[p]["pose_T"]) and np.array_equal(X, probs[p]["pt_X"])


def test_draining_thousands_of_workgroups(built):
    """4000 workgroups (256 threads at about 250 VGPRs: one wave per SIMD, so one
    workgroup per CU and 256 on the device) are many times what is resident at once: the
    batch drains, and every copy gives the bits of the first."""
    two = [scenes.scaled_problem(window(3, 20, True, 41, n_fixed=1)),
           scenes.scaled_problem(window(3, 19, False, 42, n_fixed=1))]
    kw = dict(FIXED, max_iter=3)
    got = solve_batch(two * 2000, kw)
    for p, g in enumerate(got):
        f = got[p % 2]
        assert g[1].status == 0 and g[1].n_iter == 3
        assert np.array_equal(g[2], f[2]) and np.array_equal(g[3], f[3])
        assert np.array_equal(row_bits(g[0]), row_bits(f[0]))
    o = O.Oracle(two[0])
    orows, _ = o.solve(O.make_options(**kw))
    check_against(got[0], orows, o.get_poses(), o.get_points())


def test_update_values_and_resolve(five):
    probs, _, _ = five
    rng = np.random.default_rng(9)
    pert = copy.deepcopy(probs[:3])
    for pr in pert:
        free = pr["pose_fixed"] == 0
        pr["pose_T"] = pr["pose_T"].copy()
        pr["pose_T"][free, 9:] += rng.uniform(-2e-4, 2e-4, (int(free.sum()), 3))
        pr["pt_X"] = pr["pt_X"] + rng.uniform(-5e-4, 5e-4, pr["pt_X"].shape)
    fresh = solve_batch(pert, FIXED)
    b = BaBatch(probs[:3])
    b.solve(make_options(**FIXED))
    b.update_values(np.concatenate([p["pose_T"] for p in pert]),
                    np.concatenate([p["pt_X"] for p in pert]))
    rows, res = b.solve(make_options(**FIXED))
    T, X = b.get_poses(), b.get_points()
    for p in range(3):
        assert np.array_equal(b.poses_of(p, T), fresh[p][2])
        assert np.array_equal(b.points_of(p, X), fresh[p][3])
        assert np.array_equal(row_bits(rows[p]), row_bits(fresh[p][0]))
    info = b.info()
    assert info["max_opt_poses"] == 16 and info["max_poses"] == 64 and info["max_cameras"] == 8
    assert info["image_columns"] == 64 and info["lds_bytes"] < 160 * 1024 and info["B"] == 3
    # per problem: 18 doubles per optimisable landmark (C, b, Cinv, Cinv b) and per pair (W),
    # 3 per point (trial points); no point of these problems is fixed
    want = []
    for pr in probs[:3]:
        free = np.nonzero(pr["pose_fixed"] == 0)[0]
        m = np.isin(pr["obs_pose"], free)
        pairs = np.unique(pr["obs_pt"][m].astype(np.int64) * 64 + pr["obs_pose"][m]).size
        want.append(8 * (21 * len(pr["pt_X"]) + 18 * pairs))
    assert info["scratch_bytes"] == want and info["scratch_bytes_max"] == max(want)
    b.close()


STOP_SCENES = [((5, 31, False, 328), dict(pose_noise=0.05, point_noise=0.2)),
               ((6, 40, False, 320), dict(pose_noise=0.2, point_noise=1.0)),
               ((8, 50, False, 313), dict(pose_noise=0.2, point_noise=1.0))]
STOP_THR = 1e-5                                  # default threshold of step and of cost change


def stop_margins(orows):
    """(the smaller deciding quantity over its threshold at the stopping iteration, the
    smallest such ratio over the iterations before it).  The stop rule compares the
    row's abs_step and |trial cost - previous trial cost| with the two thresholds."""
    q = [min(r.abs_step, abs(r.trial_cost - prev.trial_cost)) / STOP_THR
         for prev, r in zip(orows[:-1], orows[1:])]
    return q[-1], min([orows[0].abs_step / STOP_THR] + q[:-1])


def test_own_stop_rule(built):
    """One batch runs with the default thresholds (1e-5 / 1e-5) until each problem
    stops by itself; n_iter and converged must equal the oracle's.

    Scenes: three noise-free mono windows of ba_batch_scene, 5 / 6 / 8 poses with 31 /
    40 / 50 landmarks, seeds 328 / 320 / 313, pose noise 0.05 / 0.2 / 0.2 m, point noise
    0.2 / 1.0 / 1.0 m, solved with initial lambda 1e-6: with so little damping the
    iteration is Gauss-Newton on a zero-residual problem and converges quadratically, so
    one iteration shrinks the step by a factor of several hundred.  (With the default
    lambda 100 the step shrinks 4..25x per iteration near the stop, and stereo windows
    converge slowly whatever lambda is, because the last-writer rule drops one of the two
    cross blocks of every pair: no such scene has a stop that is not marginal.)

    Margins on the CPU oracle: the stop is decided by abs_step after 3 / 4 / 4
    iterations, where it is 0.045 / 0.046 / 0.041 of its threshold; one iteration
    earlier it is 12.4 / 19.9 / 14.6 times the threshold, and the cost change is above
    40 times its threshold throughout.  The test asserts these margins (below a tenth,
    above ten times) on the oracle's rows before it compares."""
    probs = [scenes.scaled_problem(window(*a, **k)) for a, k in STOP_SCENES]
    kw = dict(max_iter=50, lambda0=1e-6)        # default thresholds 1e-5 / 1e-5
    got = solve_batch(probs, kw)
    for p, pr in enumerate(probs):
        o = O.Oracle(pr)
        orows, oconv = o.solve(O.make_options(**kw))
        assert oconv and 3 <= len(orows) < 50
        at_stop, before = stop_margins(orows)
        print("problem %d: oracle %d iterations, batch %d; deciding quantity %.3f of its "
              "threshold at the stop, %.1f times before" % (p, len(orows), got[p][1].n_iter,
                                                           at_stop, before))
        assert at_stop < 0.1 and before > 10.0
        assert got[p][1].n_iter == len(orows) and bool(got[p][1].converged) == oconv
        assert_same_trajectory(got[p][0], orows)


def _solver_for(sc):
    s = FullBundleAdjustmentSolver(0)
    for c in range(sc["intr"].shape[0]):
        s.AddCamera(c, Camera(*sc["intr"][c], pose_this_to_cam0=sc["T_cj"][c]))
    poses = sc["T_wc_init"].copy()
    pts = sc["X_init"].copy()
    hp = s.AddPoseArray(poses)
    hq = s.AddPointArray(pts)
    for j in np.nonzero(sc["pose_fixed"])[0]:
        s.MakePoseFixed(int(hp[j]))
    for c in range(sc["intr"].shape[0]):
        m = sc["obs_cam"] == c
        s.AddObservations(c, hp[sc["obs_pose"][m]], hq[sc["obs_pt"][m]], sc["obs_uv"][m])
    return s, poses, pts


def test_python_solve_batch_matches_three_solves(built):
    scs = [window(5, 31, True, 51), window(4, 27, False, 52), window(6, 35, True, 53)]
    opt = Options()
    opt.iteration_handle.max_num_iterations = ITERS
    opt.convergence_handle.threshold_step_size = 0.0
    opt.convergence_handle.threshold_cost_change = 0.0
    single = []
    for sc in scs:
        s, poses, pts = _solver_for(sc)
        sm = Summary()
        s.Solve(opt, sm)
        single.append((poses, pts, sm))
    objs = [_solver_for(sc) for sc in scs]
    sums = [Summary() for _ in scs]
    res = FullBundleAdjustmentSolver.SolveBatch([o[0] for o in objs], opt, sums)
    for k in range(3):
        assert res[k].status == 0 and res[k].n_iter == ITERS
        assert relerr(objs[k][1], single[k][0]) < 1e-6 and relerr(objs[k][2], single[k][1]) < 1e-6
        assert not np.array_equal(objs[k][2], scs[k]["X_init"])
        a, b = sums[k].optimization_info_list_, single[k][2].optimization_info_list_
        assert len(a) == len(b) == ITERS
        for x, y in zip(a, b):
            assert x.iteration_status == y.iteration_status
            assert relerr(x.trial_cost, y.trial_cost) < 1e-7
