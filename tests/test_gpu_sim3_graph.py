"""GPU tests of the Sim(3) pose-graph optimisation (ba_sim3_*, BaSim3Graph, AddRelativeSim3 /
SolveSim3Graph; csrc/ba_sim3.hip).

Reference: sim3_ref.lm (numpy fp64, scipy expm / logm, dense solve) on the seeded graphs of
sim3_cases.py, whose fitness for a trajectory comparison test_sim3_ref.py pins without a GPU.

Sizes: 2 poses with one optimisable; N = 4, 5, 9, 10 optimisable poses with BA_DENSE_NB = 32 and
64 (4 / 9 poses fill a tile, one more starts the next); 31 / 32 / 33 factors around one k_s3_lin
workgroup (the count ba_sim3_info reports); 60 poses: more than 96 columns, several levels, fill
from closures, a pair named twice in both orientations, a fixed pose as j and as k.

Tolerances: H and g 1e-9 relative (the project's for get_S), the cost 1e-12 relative; status and
lambda equal, costs 1e-7 relative; final poses max_j |sim3_log(S_gpu S_ref^-1)| <= 10 noise +
1e-13, noise the same distance between the reference's two host solves (numpy.linalg.solve and
a scipy Cholesky); the noise-free scenes reach the truth to 1e-8.
"""
import ctypes as C

import numpy as np
import pytest

from bundle_adjustment_solver_amd._lib import BaIterInfo, make_options
from bundle_adjustment_solver_amd.solver import (INVERSE_SCALER, BaPoseGraph, BaProblem, BaSim3Graph, Camera,
                                                 FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor,
                                                 Options, Summary, _T12_to_44, rigid_inverse)
from bundle_adjustment_solver_amd import scenes

import pgo_cases
import sim3_cases as cases
import sim3_ref

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def make(name, owner=None):
    g = cases.scene(name)
    return BaSim3Graph(g["pose_S"], g["pose_fixed"], g["rels"], owner=owner)


def assert_same_trajectory(rows, orows, rtol_cost=1e-7):
    """identical decisions, lambda to 1e-12, cost and trial cost to rtol_cost (floored at 1e-12
    of the first cost)"""
    assert len(rows) == len(orows)
    floor = 1e-12 * abs(orows[0].cost)
    for k, (a, b) in enumerate(zip(rows, orows)):
        assert a.iteration_status == b.iteration_status, k
        assert relerr(a.damping_term, b.damping_term) < 1e-12, k
        assert abs(a.trial_cost - b.trial_cost) <= rtol_cost * abs(b.trial_cost) + floor, k
        assert abs(a.cost - b.cost) <= rtol_cost * abs(b.cost) + floor, k


def assert_poses(what, S, ref_S, chol_S, info):
    noise = sim3_ref.pose_distance(chol_S, ref_S)
    err = sim3_ref.pose_distance(S, ref_S)
    print("%s final poses: error %.3e, noise of the host reference %.3e, ratio %.2f, pivots %d"
          % (what, err, noise, err / max(noise, 1e-300), info["bad_pivots"]))
    assert noise <= 1e-8, "scene unfit: the two host references disagree"
    assert err <= 10.0 * noise + 1e-13
    assert info["bad_pivots"] == 0


def check_trajectory(name, p):
    ref_rows, ref_conv, ref_S = cases.reference(name)
    rows, conv = p.solve(cases.options(name))
    for k, (a, b) in enumerate(zip(rows, ref_rows)):
        print("%s it %d: status %d/%d lambda %.6g/%.6g trial %.12g/%.12g cost %.12g/%.12g rho %.4g/%.4g"
              % (name, k, a.iteration_status, b.iteration_status, a.damping_term, b.damping_term,
                 a.trial_cost, b.trial_cost, a.cost, b.cost, a.rho, b.rho))
    assert_same_trajectory(rows, ref_rows)
    assert conv == ref_conv
    for a, b in zip(rows, ref_rows):   # the other columns of the rows, as the definition states them
        assert abs(a.rho - b.rho) <= 1e-6 * max(1.0, abs(b.rho))
        assert abs(a.model_change - b.model_change) <= 1e-7 * abs(b.model_change)
        assert abs(a.abs_step - b.abs_step) <= 1e-7 * abs(b.abs_step)
        # cost_change = |accepted - trial|: each of the two to 1e-7 relative, and the accepted
        # chi-square before the step is at most trial + change (on g2 it is 4 000 times the trial cost)
        assert abs(a.cost_change - b.cost_change) <= \
            1e-7 * (abs(b.trial_cost) + abs(b.cost_change)) + 1e-12 * ref_rows[0].cost
        assert abs(a.average_reprojection_error - b.average_reprojection_error) <= 1e-7 * b.average_reprojection_error
    assert_poses(name, p.poses(), ref_S, cases.reference_cholesky(name)[2], p.info())


# ---- 1. system and cost -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g2", "n10", "g30_31", "g30_32", "g30_33", "g60"])
def test_system_and_cost_match_the_host_statement(built, name):
    g = cases.scene(name)
    p = make(name)
    H, gr = p.system()
    rH, rg = sim3_ref.dense_system(g["pose_fixed"], g["pose_S"], g["rels"])
    terms = sim3_ref.chi2_terms(g["pose_S"], g["rels"])
    c, rc = p.cost(), sim3_ref.chi2(g["pose_S"], g["rels"])
    info = p.info()
    print(name, info, "H", relerr(H, rH), "g", relerr(gr, rg), "cost", abs(c - rc) / rc)
    assert info["N"] == int((g["pose_fixed"] == 0).sum()) and info["factors"] == len(g["rels"]["j"])
    assert relerr(H, rH) < 1e-9 and relerr(gr, rg) < 1e-9
    assert np.array_equal(H, H.T)
    assert abs(c - rc) <= 1e-12 * rc
    assert relerr(p.factor_report(), terms) < 1e-9
    assert np.array_equal(p.poses(), g["pose_S"])   # none of the calls moves the poses
    p.close()


# ---- 2. trajectories ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g2", "g30_31", "g30_32", "g30_33", "g60_63", "g60", "g60_gn"])
def test_trajectory_matches_the_reference(built, name):
    p = make(name)
    info = p.info()
    if name.startswith("g30_"):   # one factor short of a k_s3_lin workgroup, a full one, one over
        assert info["factors"] - info["fpb"] == {"g30_31": -1, "g30_32": 0, "g30_33": 1}[name]
    check_trajectory(name, p)
    if name == "g60":
        assert info["nb"] * info["tiles"] > 96 and info["levels"] >= 2   # non-tail levels and the sweeps ran
        assert info["blocks"] > info["N"] - 1                           # closures: blocks off the chain
    p.close()


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("name", ["n4", "n5", "n9", "n10"])
def test_pose_per_tile_edges(built, monkeypatch, name, nb):
    """N = 4, 5, 9, 10 optimisable poses: a full tile of 4 / 9 poses, one pose into the next"""
    monkeypatch.setenv("BA_DENSE_NB", str(nb))   # read by ba_create
    p = make(name)
    monkeypatch.delenv("BA_DENSE_NB")
    info = p.info()
    ppt = nb // 7
    assert info["nb"] == nb and info["tiles"] == (info["N"] + ppt - 1) // ppt
    check_trajectory(name, p)
    p.close()


# ---- 3. noise-free scenes: the small-angle and small-sigma branches on the device ---------------
@pytest.mark.parametrize("name", sorted(cases.EXACT))
def test_noise_free_scene_reaches_the_truth(built, name):
    g = cases.scene(name)
    p = make(name)
    rows, _ = p.solve(make_options(max_iter=8, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4))
    err = sim3_ref.pose_distance(p.poses(), g["truth"])
    print(name, "distance to the truth", err, "chi2", rows[-1].cost, "largest s_f", p.factor_report().max())
    assert err <= 1e-8
    p.close()


# ---- 4. stop ------------------------------------------------------------------------------------
def test_stop_test_matches_the_reference(built):
    ref_rows, ref_conv, ref_S = cases.stop_reference()
    assert ref_conv and len(ref_rows) < cases.STOP["opt"]["max_iter"]
    p = make(cases.STOP["scene"])
    cap = cases.STOP["opt"]["max_iter"]
    buf = (BaIterInfo * cap)()
    C.memset(buf, 0xAB, C.sizeof(buf))
    rows, conv = p.solve(make_options(**cases.STOP["opt"]), cap=cap, rows=buf)
    print("stopped after", p.n_iter, "iterations; the reference after", len(ref_rows))
    assert p.n_iter == len(ref_rows) and conv == ref_conv
    untouched = bytes(buf)[p.n_iter * C.sizeof(BaIterInfo):]
    assert untouched == b"\xab" * len(untouched)   # rows beyond n_iter are untouched
    assert_poses("stop", p.poses(), ref_S, cases.stop_reference_cholesky()[2], p.info())
    p.close()


def test_a_single_iteration_never_reports_convergence(built):
    p = make(cases.STOP["scene"])
    rows, conv = p.solve(make_options(max_iter=1, thr_step=1e30, thr_cost=1e30, lambda0=1e-4))
    assert len(rows) == 1 and not conv
    rows, conv = p.solve(make_options(max_iter=2, thr_step=1e30, thr_cost=1e30, lambda0=1e-4))
    assert len(rows) == 1 and conv   # the first of two allowed iterations may stop
    p.close()


# ---- 5. determinism and state -------------------------------------------------------------------
def row_bits(rows):
    return [(r.cost, r.trial_cost, r.damping_term, r.rho, r.model_change, r.abs_step, r.iteration_status)
            for r in rows]


def test_same_bits_run_to_run_and_after_update_values(built):
    g = cases.scene("g60")
    opt = cases.options("g60", max_iter=6)
    p = make("g60")
    r1, _ = p.solve(opt)
    S1 = p.poses()
    assert not np.array_equal(S1, g["pose_S"])
    p.update_values(g["pose_S"])
    r2, _ = p.solve(opt)
    assert row_bits(r1) == row_bits(r2) and np.array_equal(S1, p.poses())
    # new values for the same structure: equal to a fresh object, to the bit
    h = cases.graph(**dict(cases.SCENES["g60"][0], drift=1.0))
    assert np.array_equal(h["rels"]["j"], g["rels"]["j"]) and not np.array_equal(h["pose_S"], g["pose_S"])
    Z2 = h["rels"]["Z"]
    Om2 = 0.5 * h["rels"]["Omega"]
    p.update_values(h["pose_S"], Z2, Om2)
    r3, _ = p.solve(opt)
    S3 = p.poses()
    q = BaSim3Graph(h["pose_S"], h["pose_fixed"], dict(h["rels"], Z=Z2, Omega=Om2))
    r4, _ = q.solve(opt)
    assert row_bits(r3) == row_bits(r4) and np.array_equal(S3, q.poses())
    assert row_bits(r3) != row_bits(r1)
    # a refused update changes nothing
    bad = Z2.copy()
    bad[3, 12] = 0.0
    with pytest.raises(Exception, match="factor 3"):
        p.update_values(None, bad, None)
    assert np.array_equal(p.poses(), S3) and p.cost() == q.cost()
    p.close()
    q.close()


HUBER = 1   # ba_hip.h: BA_ROBUST_HUBER


def graph_calls(p, g, opt, opt1, huber):
    """The calls of one graph between the solves of the others, one per step, each returning what
    it computed: solve, covariance (three poses, two pairs) and gate (two candidates) at the solved
    poses; then Huber on every factor (huber) or nothing, a one-iteration solve, and covariance,
    gate and the poses again, and the dropped pivots of the last solve and of the last gate.  The pairs and the candidates are the graph's first two factors."""
    r = g["rels"]
    sel = np.flatnonzero(np.asarray(g["pose_fixed"]) == 0)[:3].astype(np.int32)
    pairs = (np.asarray(r["j"][:2], np.int32), np.asarray(r["k"][:2], np.int32))
    cand = (r["j"][:2], r["k"][:2], r["Z"][:2], r["Omega"][:2])
    return [lambda: row_bits(p.solve(opt)[0]),
            lambda: p.covariance(sel, pairs),
            lambda: p.gate(*cand),
            lambda: p.set_robust(np.full(p.n_rel, HUBER, np.int32), np.full(p.n_rel, 1.5)) if huber else None,
            lambda: row_bits(p.solve(opt1)[0]),
            lambda: p.covariance(sel, pairs),
            lambda: p.gate(*cand),
            lambda: p.poses(),
            lambda: (p.info()["bad_pivots"], p.dropped_pivots)]


def same_bits(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


def test_a_solve_leaves_the_other_users_of_a_handle_alone(built):
    """a full-BA trajectory on a second handle, and an SE(3) BaPoseGraph on the SAME handle, to the
    bit; and two Sim(3) graphs and an SE(3) graph that borrow one handle and take turns at solve,
    covariance, gate and set_robust each return the bits of the same calls on a graph alone on a
    fresh handle.  The two kinds share the code that moves allocations between the handle and a
    graph (the graph's own, the robust arrays, the scratch of a covariance call) and the code that
    saves and restores the controller and the count of dropped pivots.  n10 and g12: 12 poses;
    g30_33: two or more tiles at order 32, k_s3_lin workgroups of 32 factors."""
    sc = scenes.synthetic_ba_scene(12, 300, 5, True, seed=7)
    pr = scenes.scaled_problem(sc)

    def ba():
        b = BaProblem(0)
        b.set_cameras(pr["cam_intr"], pr["cam_T"])
        b.set_poses(pr["pose_T"], pr["pose_fixed"])
        b.set_points(pr["pt_X"], pr["pt_fixed"])
        b.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
        b.finalize()
        return b

    def se3(owner):
        g = pgo_cases.scene("g12")
        return BaPoseGraph(g["pose_T"], g["pose_fixed"], g["rels"], owner=owner)

    # (make the graph, its scene, its options, Huber in the middle): Huber on one graph of each
    # kind, the third stays plain
    users = [(lambda o: make("n10", owner=o), cases.scene("n10"), cases.options, "n10", True),
             (se3, pgo_cases.scene("g12"), pgo_cases.options, "g12", True),
             (lambda o: make("g30_33", owner=o), cases.scene("g30_33"), cases.options, "g30_33", False)]

    def calls_of(user, owner):
        mk, g, options, name, huber = user
        p = mk(owner)
        return p, graph_calls(p, g, options(name), options(name, max_iter=1), huber)

    alone = []
    for user in users:   # each graph alone on a fresh handle of its own
        p, calls = calls_of(user, None)
        alone.append([c() for c in calls])
        p.close()

    opt = make_options(max_iter=4, thr_step=0.0, thr_cost=0.0)
    a = ba()
    rows_a, _ = a.solve(opt)
    Ta, Xa = a.get_poses(), a.get_points()[0]
    e = se3(a)
    rows_e, _ = e.solve(pgo_cases.options("g12"))
    Te = e.poses()
    e.close()
    a.close()
    b = ba()
    p = make("g60")            # a Sim(3) graph on a handle of its own ...
    q = make("n10", owner=b)   # ... one that borrows the handle of the problem ...
    f = se3(b)                 # ... and an SE(3) graph on that same handle
    p.solve(cases.options("g60", max_iter=3))
    q.solve(cases.options("n10"))
    rows_f, _ = f.solve(pgo_cases.options("g12"))
    q.solve(cases.options("n10"))
    assert row_bits(rows_e) == row_bits(rows_f) and np.array_equal(Te, f.poses())
    # the three users on the problem's handle, one call each in turn
    shared = [calls_of(user, b) for user in users]
    got = [[] for _ in users]
    for step in range(len(shared[0][1])):
        for u, (_, calls) in enumerate(shared):
            got[u].append(calls[step]())
    for u, (g, _) in enumerate(shared):
        for step, (x, y) in enumerate(zip(got[u], alone[u])):
            assert same_bits(x, y), (users[u][3], step)
    rows_b, _ = b.solve(opt)
    assert [(r.trial_cost, r.iteration_status) for r in rows_a] == [(r.trial_cost, r.iteration_status) for r in rows_b]
    assert np.array_equal(Ta, b.get_poses()) and np.array_equal(Xa, b.get_points()[0])
    for g, _ in shared:
        g.close()
    f.close()
    q.close()
    p.close()
    b.close()


# ---- 6. facade ----------------------------------------------------------------------------------
def facade(cls, sc, se3_factors=True, sim3_factors=True):
    s = cls()
    s.AddCamera(0, Camera(*sc["camera"]))
    poses, pts = sc["poses"].copy(), sc["points"].copy()
    hp = s.AddPoseArray(poses)
    hq = s.AddPointArray(pts)
    s.MakePoseFixed(int(hp[0]))
    s.AddObservations(0, hp[sc["obs"][0]], hq[sc["obs"][1]], sc["obs"][2])
    if sim3_factors:
        for j, k, M, Om in sc["factors"]:
            s.AddRelativeSim3(int(hp[j]), int(hp[k]), M, Om, sigma_pixel=0.7)
    if se3_factors:   # rigid odometry of the drifted map, for SolvePoseGraph
        rng = np.random.default_rng(3)
        for j, k, M, Om in sc["factors"][:len(poses) - 1]:
            R = M.copy()
            R[:3, :3] /= np.cbrt(np.linalg.det(M[:3, :3]))
            R[:3, 3] += 1e-2 * rng.standard_normal(3)
            s.AddRelativePose(int(hp[j]), int(hp[k]), R, Om[:6, :6], sigma_pixel=0.7)
    return s, poses, pts


def facade_options(n=7):
    options = Options()
    options.iteration_handle.max_num_iterations = n
    options.convergence_handle.threshold_step_size = -1.0
    options.convergence_handle.threshold_cost_change = -1.0
    options.trust_region_handle.initial_lambda = 1e-4
    return options


@pytest.mark.parametrize("cls", [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor])
def test_facade_is_the_raw_call_and_keeps_the_anchored_projections(built, cls):
    sc = cases.loop_scene()
    s, poses, pts = facade(cls, sc)
    start, pts0 = poses.copy(), pts.copy()
    s.FinalizeParameters()   # a finalized problem of the same solver: it takes the result below
    options = facade_options()
    T0 = np.concatenate(s._pose_T_jw, axis=0)
    pf = np.zeros(len(T0), np.uint8)
    pf[list(s._pose_fixed)] = 1
    c_opt = options.to_c()
    c_opt.gauss_newton = 1 if s._use_gauss_newton(options) else 0
    S0 = np.c_[T0, np.ones(len(T0))]
    rels = s._sim3_arrays()
    raw = BaSim3Graph(S0, pf, rels)
    rows, conv = raw.solve(c_opt)
    S_raw = raw.poses()
    raw.close()
    before = cases.project(sc["camera"], start[sc["anchors"]], pts0)
    summary = Summary()
    scales = s.SolveSim3Graph(options, summary, point_anchors=list(sc["anchors"]))
    got = summary.optimization_info_list_
    assert [(r.cost, r.trial_cost, r.damping_term, r.iteration_status) for r in rows] == \
        [(r.cost, r.trial_cost, r.damping_term, int(r.iteration_status)) for r in got]
    assert len(rows) == 7 and not conv and summary.convergence_status_ is False
    # the poses went back rigid, T_jw = [R, t / s], through the unit conversion of Solve
    assert np.array_equal(scales, S_raw[:, 12])
    T_new = S_raw[:, :12].copy()
    T_new[:, 9:12] /= S_raw[:, 12:13]
    T44 = _T12_to_44(T_new)
    T44[:, :3, 3] *= INVERSE_SCALER
    want = rigid_inverse(T44)
    assert np.array_equal(poses[1:], want[1:]) and not np.array_equal(poses[1:], start[1:])
    assert np.array_equal(poses[0], start[0]) and scales[0] == 1.0
    RtR = np.einsum("nji,njk->nik", poses[:, :3, :3], poses[:, :3, :3])
    assert np.abs(RtR - np.eye(3)).max() <= 1e-12 and np.all(poses[:, 3] == [0.0, 0.0, 0.0, 1.0])
    assert np.array_equal(np.concatenate(s._pose_T_jw, axis=0), T_new)
    # every anchored point reprojects into its anchor keyframe where it did before
    after = cases.project(sc["camera"], poses[sc["anchors"]], pts)
    print("largest reprojection shift of an anchored point: %.3e px" % np.abs(after - before).max())
    assert np.abs(after - before).max() <= 1e-9 and not np.array_equal(pts, pts0)
    # the scales against the reference on the same scaled arrays, by the rule of the final poses
    ref = dict(pose_S=S0, pose_fixed=pf, rels=rels)
    ref_S = sim3_ref.lm(ref, c_opt)[2]
    chol_S = sim3_ref.lm(ref, c_opt, sim3_ref.solve_cholesky)[2]
    noise = sim3_ref.pose_distance(chol_S, ref_S)
    err = sim3_ref.pose_distance(S_raw, ref_S)
    tol = 10.0 * noise + 1e-13
    print("facade scene: error %.3e, noise %.3e; scales off the reference by %.3e, off the injected drift by %.3e"
          % (err, noise, np.abs(np.log(scales / ref_S[:, 12])).max(), np.abs(np.log(scales / sc["scale"])).max()))
    assert noise <= 1e-8 and err <= tol
    assert np.abs(np.log(scales / ref_S[:, 12])).max() <= tol
    assert np.abs(np.log(scales / sc["scale"])).max() <= np.abs(np.log(ref_S[:, 12] / sc["scale"])).max() + tol
    # the finalized problem of the same solver takes the new poses and points
    s.ReloadParameterValues()
    T_problem = s._problem.get_poses()
    X_problem = s._problem.get_points()[0]
    assert np.abs(T_problem - T_new).max() <= 1e-9 * max(1.0, np.abs(T_new).max())
    assert np.abs(X_problem - np.concatenate(s._pt_X, axis=0)).max() <= 1e-9
    assert np.abs(T_problem - T0).max() > 1e-6


@pytest.mark.parametrize("cls", [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor])
def test_each_solve_uses_its_own_kind_of_factor(built, cls):
    sc = cases.loop_scene()
    both, poses_b, _ = facade(cls, sc)
    only, poses_o, _ = facade(cls, sc, sim3_factors=False)
    sa, sb = Summary(), Summary()
    assert both.SolvePoseGraph(facade_options(4), sa) is True
    assert only.SolvePoseGraph(facade_options(4), sb) is True
    assert [(r.cost, r.trial_cost) for r in sa.optimization_info_list_] == \
        [(r.cost, r.trial_cost) for r in sb.optimization_info_list_]
    assert np.array_equal(poses_b, poses_o) and not np.array_equal(poses_b, sc["poses"])
    # and the Sim(3) solve sees no SE(3) factor
    both2, poses_2, _ = facade(cls, sc)
    only2, poses_3, _ = facade(cls, sc, se3_factors=False)
    s2 = both2.SolveSim3Graph(facade_options(4))
    s3 = only2.SolveSim3Graph(facade_options(4))
    assert np.array_equal(s2, s3) and np.array_equal(poses_2, poses_3)
    with pytest.raises(RuntimeError, match="AddRelativeSim3"):
        only.SolveSim3Graph(facade_options(4))
