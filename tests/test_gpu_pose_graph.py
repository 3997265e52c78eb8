"""GPU tests of the pose-graph optimisation (ba_pgraph_*, BaPoseGraph, SolvePoseGraph;
csrc/ba_pgraph.hip).

Reference: pgo_ref.lm (numpy fp64, dense solve) on the seeded graphs of pgo_cases.py, whose
fitness for a trajectory comparison (no gain ratio near a threshold, every iteration moves
chi-square, all three statuses) test_pgo_ref.py pins without a GPU.

Sizes: 2, 12, 60 and 330 poses, the smallest that reach one optimisable pose, the
pose-per-tile edges (N = 5, 6, 10, 11, each with BA_DENSE_NB=32 and 64), more than 96 columns
(non-tail levels and the sweeps), 63 / 64 / 65 factors around one k_pg_lin workgroup of 64, and
several levels with fill from closures.

Tolerances: H and g 1e-9 relative (the project's for get_S), the cost 1e-12 relative; the
trajectory rule of test_gpu_parity.assert_same_trajectory restated (status identical, lambda
1e-12, cost and trial cost 1e-7 relative); final poses max_j |se3_log(T_gpu T_ref^-1)| <=
10 max(noise, 1e-12) with noise the same distance between two host runs of the reference
(numpy.linalg.solve against a scipy Cholesky solve), the scene unfit if noise > 1e-8.
"""
import ctypes as C

import numpy as np
import pytest

from bundle_adjustment_solver_amd._lib import BaIterInfo, make_options
from bundle_adjustment_solver_amd.solver import (INVERSE_SCALER, BaPoseGraph, BaProblem, FullBundleAdjustmentSolver,
                                                 FullBundleAdjustmentSolverRefactor, Options, _T12_to_44,
                                                 rigid_inverse)
from bundle_adjustment_solver_amd import scenes

import pgo_cases as cases
import pgo_ref
import rel_ref

pytestmark = pytest.mark.gpu


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def make(name):
    g = cases.scene(name)
    return BaPoseGraph(g["pose_T"], g["pose_fixed"], g["rels"])


def assert_same_trajectory(rows, orows, rtol_cost=1e-7):
    """test_gpu_parity.assert_same_trajectory: identical decisions, lambda to 1e-12, cost and
    trial cost to rtol_cost (floored at 1e-12 of the first cost)"""
    assert len(rows) == len(orows)
    floor = 1e-12 * abs(orows[0].cost)
    for k, (a, b) in enumerate(zip(rows, orows)):
        assert a.iteration_status == b.iteration_status, k
        assert relerr(a.damping_term, b.damping_term) < 1e-12, k
        assert abs(a.trial_cost - b.trial_cost) <= rtol_cost * abs(b.trial_cost) + floor, k
        assert abs(a.cost - b.cost) <= rtol_cost * abs(b.cost) + floor, k


def check_trajectory(name, p):
    ref_rows, ref_conv, ref_T = cases.reference(name)
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
        assert abs(a.cost_change - b.cost_change) <= 1e-7 * abs(b.cost) + 1e-12 * ref_rows[0].cost
        assert abs(a.average_reprojection_error - b.average_reprojection_error) <= 1e-7 * b.average_reprojection_error
    noise = pgo_ref.pose_distance(cases.reference_cholesky(name)[2], ref_T)
    assert noise <= 1e-8, "scene unfit: the two host references disagree"
    err = pgo_ref.pose_distance(p.poses(), ref_T)
    print("%s final poses: error %.3e, noise of the host reference %.3e, pivots %d"
          % (name, err, noise, p.info()["bad_pivots"]))
    assert err <= 10.0 * max(noise, 1e-12)
    assert p.info()["bad_pivots"] == 0


# ---- 1. system and cost -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g2", "g12", "g60_63", "g60", "g60_65", "g330"])
def test_system_and_cost_match_the_host_statement(built, name):
    g = cases.scene(name)
    p = make(name)
    H, gr = p.system()
    rH, rg = rel_ref.dense_factors(dict(pose_fixed=g["pose_fixed"]), g["pose_T"], g["rels"])
    c, rc = p.cost(), pgo_ref.chi2(g["pose_T"], g["rels"])
    info = p.info()
    print(name, info, "H", relerr(H, rH), "g", relerr(gr, rg), "cost", abs(c - rc) / rc)
    assert info["N"] == int((g["pose_fixed"] == 0).sum()) and info["factors"] == len(g["rels"]["j"])
    assert relerr(H, rH) < 1e-9 and relerr(gr, rg) < 1e-9
    assert np.array_equal(H, H.T)
    assert abs(c - rc) <= 1e-12 * rc
    assert np.array_equal(p.poses(), g["pose_T"])   # neither call moves the poses
    p.close()


# ---- 2. trajectories ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g2", "g12", "g60_63", "g60", "g60_65", "g60_gn", "g60_hard_gn", "g330"])
def test_trajectory_matches_the_reference(built, name):
    p = make(name)
    check_trajectory(name, p)
    if name == "g60":
        assert p.info()["nb"] * p.info()["tiles"] > 96   # non-tail levels and the sweeps ran
    if name == "g330":
        assert p.info()["levels"] > 2
    p.close()


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("name", ["n5", "n6", "n10", "g12"])
def test_pose_per_tile_edges(built, monkeypatch, name, nb):
    """N = 5, 6, 10, 11 optimisable poses: a full tile of 5 / 10 poses, one pose into the next"""
    monkeypatch.setenv("BA_DENSE_NB", str(nb))   # read by ba_create
    p = make(name)
    monkeypatch.delenv("BA_DENSE_NB")
    info = p.info()
    ppt = 5 if nb == 32 else 10
    assert info["nb"] == nb and info["tiles"] == (info["N"] + ppt - 1) // ppt
    check_trajectory(name, p)
    p.close()


# ---- 3. stop ------------------------------------------------------------------------------------
def test_stop_test_matches_the_reference(built):
    ref_rows, ref_conv, ref_T = cases.stop_reference()
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
    # the final poses by the rule of the trajectories: ten times the reference's own noise
    noise = pgo_ref.pose_distance(
        pgo_ref.lm(cases.scene(cases.STOP["scene"]), make_options(**cases.STOP["opt"]), pgo_ref.solve_cholesky)[2], ref_T)
    err = pgo_ref.pose_distance(p.poses(), ref_T)
    print("final poses: error %.3e, noise of the host reference %.3e" % (err, noise))
    assert noise <= 1e-8 and err <= 10.0 * max(noise, 1e-12)
    p.close()


def test_a_single_iteration_never_reports_convergence(built):
    p = make(cases.STOP["scene"])
    rows, conv = p.solve(make_options(max_iter=1, thr_step=1e30, thr_cost=1e30, lambda0=1e-4))
    assert len(rows) == 1 and not conv
    rows, conv = p.solve(make_options(max_iter=2, thr_step=1e30, thr_cost=1e30, lambda0=1e-4))
    assert len(rows) == 1 and conv   # the first of two allowed iterations may stop
    p.close()


# ---- 4. determinism and state -------------------------------------------------------------------
def row_bits(rows):
    return [(r.cost, r.trial_cost, r.damping_term, r.rho, r.model_change, r.abs_step, r.iteration_status)
            for r in rows]


def test_same_bits_run_to_run_and_after_update_values(built):
    g = cases.scene("g330")
    opt = cases.options("g330", max_iter=6)
    p = make("g330")
    r1, _ = p.solve(opt)
    T1 = p.poses()
    assert not np.array_equal(T1, g["pose_T"])
    p.update_values(g["pose_T"])
    r2, _ = p.solve(opt)
    T2 = p.poses()
    assert row_bits(r1) == row_bits(r2) and np.array_equal(T1, T2)
    # new values for the same structure: equal to a fresh object, to the bit
    h = cases.graph(**dict(cases.SCENES["g330"][0], drift=0.2))
    assert np.array_equal(h["rels"]["j"], g["rels"]["j"]) and not np.array_equal(h["pose_T"], g["pose_T"])
    Z2 = h["rels"]["Z"]
    Om2 = 0.5 * h["rels"]["Omega"]
    p.update_values(h["pose_T"], Z2, Om2)
    r3, _ = p.solve(opt)
    T3 = p.poses()
    q = BaPoseGraph(h["pose_T"], h["pose_fixed"], dict(h["rels"], Z=Z2, Omega=Om2))
    r4, _ = q.solve(opt)
    assert row_bits(r3) == row_bits(r4) and np.array_equal(T3, q.poses())
    assert row_bits(r3) != row_bits(r1)
    # a refused update changes nothing
    bad = Z2.copy()
    bad[3, 0] = np.nan
    with pytest.raises(Exception, match="factor 3"):
        p.update_values(None, bad, None)
    assert np.array_equal(p.poses(), T3) and p.cost() == q.cost()
    p.close()
    q.close()


def test_a_solve_leaves_another_handles_problem_alone(built):
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

    opt = make_options(max_iter=4, thr_step=0.0, thr_cost=0.0)
    a = ba()
    rows_a, _ = a.solve(opt)
    Ta, Xa = a.get_poses(), a.get_points()[0]
    a.close()
    b = ba()
    p = make("g60")           # a graph on a handle of its own ...
    q = BaPoseGraph(cases.scene("g12")["pose_T"], cases.scene("g12")["pose_fixed"], cases.scene("g12")["rels"],
                    owner=b)  # ... and one that borrows the handle of the problem
    p.solve(cases.options("g60", max_iter=3))
    q.solve(cases.options("g12"))
    rows_b, _ = b.solve(opt)
    assert [(r.trial_cost, r.iteration_status) for r in rows_a] == [(r.trial_cost, r.iteration_status) for r in rows_b]
    assert np.array_equal(Ta, b.get_poses()) and np.array_equal(Xa, b.get_points()[0])
    q.close()
    p.close()
    b.close()


# ---- 5. facades ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor])
def test_facade_is_the_raw_call_on_the_scaled_arrays(built, cls):
    from test_gpu_relative import facade
    from bundle_adjustment_solver_amd.solver import Summary
    sc = scenes.synthetic_ba_scene(12, 150, 5, True, seed=12)
    nf = int(np.asarray(sc["pose_fixed"]).sum())
    pairs = [(q + 1, q) for q in range(nf - 1, 11)] + [(11, nf + 1), (nf, 9)]
    s, facs, poses, pts = facade(cls, sc, pairs, 0.7)
    start = poses.copy()
    pts0 = pts.copy()
    s.FinalizeParameters()
    options = Options()
    options.iteration_handle.max_num_iterations = 5
    options.convergence_handle.threshold_step_size = -1.0
    options.convergence_handle.threshold_cost_change = -1.0
    options.trust_region_handle.initial_lambda = 1e-4
    T0 = np.concatenate(s._pose_T_jw, axis=0)
    pf = np.zeros(len(T0), np.uint8)
    pf[list(s._pose_fixed)] = 1
    c_opt = options.to_c()
    c_opt.gauss_newton = 1 if s._use_gauss_newton(options) else 0
    raw = BaPoseGraph(T0, pf, s._relative_arrays())
    rows, conv = raw.solve(c_opt)
    T_raw = raw.poses()
    raw.close()
    summary = Summary()
    assert s.SolvePoseGraph(options, summary) is True
    got = summary.optimization_info_list_
    assert [(r.cost, r.trial_cost, r.damping_term, r.iteration_status) for r in rows] == \
        [(r.cost, r.trial_cost, r.damping_term, int(r.iteration_status)) for r in got]
    assert len(rows) == 5 and not conv and summary.convergence_status_ is False
    # the poses went back through the unit conversion of Solve, the points stayed
    T44 = _T12_to_44(T_raw)
    T44[:, :3, 3] *= INVERSE_SCALER
    want = rigid_inverse(T44)
    opt_rows = np.flatnonzero(pf == 0)
    assert np.array_equal(poses[opt_rows], want[opt_rows]) and not np.array_equal(poses[opt_rows], start[opt_rows])
    assert np.array_equal(poses[pf != 0], start[pf != 0]) and np.array_equal(pts, pts0)
    assert np.array_equal(np.concatenate(s._pose_T_jw, axis=0), T_raw)
    # the finalized problem of the same solver (same factors) takes the new poses
    s.ReloadParameterValues()
    T_problem = s._problem.get_poses()
    assert np.abs(T_problem - T_raw).max() <= 1e-9 * max(1.0, np.abs(T_raw).max())
    assert np.abs(T_problem - T0).max() > 1e-6
    assert s.Solve(options) is True
