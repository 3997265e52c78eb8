"""GPU tests of the gradient-descent loop (ba_gd_* / ba_solve_gd,
FullBundleAdjustmentSolverRefactor.SolveByGradientDescent): the gradient against
the LM linearisation, the trajectory against the numpy restatement
tests/gd_ref.py, the Python mirror and the C++ facade, determinism, no
interference with the LM loop, refusals."""
import os
import subprocess

import numpy as np
import pytest

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import BaError, make_options
from bundle_adjustment_solver_amd.solver import BaProblem

import gd_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_gpu(pr, rank=0, world=1):
    p = BaProblem(0)
    p.set_cameras(pr["cam_intr"], pr["cam_T"])
    p.set_poses(pr["pose_T"], pr["pose_fixed"])
    p.set_points(pr["pt_X"], pr["pt_fixed"])
    p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
    if world > 1:
        p.set_shard(rank, world)
    p.finalize()
    return p


def _outliers(sc, frac, px, seed):
    rng = np.random.default_rng(seed)
    sel = rng.uniform(size=len(sc["obs_uv"])) < frac
    sc["obs_uv"] = sc["obs_uv"].copy()
    sc["obs_uv"][sel] += rng.choice([-px, px], size=(int(sel.sum()), 2))
    return sc


def scene(kind):
    """(scene, huber) of every structure the GD pass has to cover."""
    if kind == "hover_fixed":          # fixed poses AND fixed points
        sc = scenes.hover_scene(8, 300, 2, seed=31, n_fixed=2)
        sc["pt_fixed"] = np.arange(300) < 40
        sc["X_init"][:40] = sc["X_true"][:40]
        return sc, 1.0
    if kind == "c2_small":             # C2 scaled down (mono, windows of 10)
        return scenes.config_scene("C2", scale=0.02), 1.0
    if kind == "stereo":
        return scenes.synthetic_ba_scene(30, 2000, 5, True, seed=41), 1.0
    if kind == "masked":               # C4R-style dropout: masked covisibility groups
        return scenes.config_scene("C4R", scale=0.01), 1.0
    if kind == "w20":                  # 20-pose windows: the ungrouped path
        return scenes.config_scene("W20", scale=0.06), 1.0
    if kind == "dense":
        return scenes.dense_covisibility_scene(30, 600, 8, seed=51), 1.0
    if kind == "huber":                # outliers of 20 px, threshold 5 px (scaled: 0.05)
        sc = scenes.synthetic_ba_scene(20, 1000, 5, True, seed=61)
        return _outliers(sc, 0.05, 20.0, seed=62), 0.05
    raise ValueError(kind)


KINDS = ["hover_fixed", "c2_small", "stereo", "masked", "w20", "dense", "huber"]


def rel_block(a, b):
    """max over blocks of |a - b| / max(|b|, tiny)."""
    a, b = np.asarray(a).reshape(len(a), -1), np.asarray(b).reshape(len(b), -1)
    den = np.maximum(np.linalg.norm(b, axis=1), 1e-300)
    return (np.linalg.norm(a - b, axis=1) / den).max() if len(a) else 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_equals_lm_linearisation(kind, built):
    sc, huber = scene(kind)
    pr = scenes.scaled_problem(sc)
    p = make_gpu(pr)
    if kind == "masked":
        mi = p.get_mask_info()
        assert mi["masked_pieces"] > 0 and mi["padded_observation_slots"] > 0, mi
    p.gd_begin(make_options(max_iter=5, huber=huber))
    a, b = p.gd_gradient()
    # (ba_options holds the threshold as float: the same value for the stage call)
    p.stage_linearize(100.0, float(np.float32(huber)))
    _, a_lm = p.get_A()
    _, b_lm = p.get_C()
    assert rel_block(a, a_lm) < 1e-12
    assert rel_block(b, b_lm) < 1e-12
    # and the restatement (summation order and vectorisation differ)
    P = gd_ref.Problem(pr)
    R, t = gd_ref.split12(pr["pose_T"])
    ar, br = gd_ref.gradient(P, R, t, pr["pt_X"].reshape(-1, 3), float(np.float32(huber)))
    assert rel_block(a, ar) < 1e-9 and rel_block(b, br) < 1e-9
    if kind == "huber":   # the threshold is active on this scene
        r = gd_ref.project(P, R, t, pr["pt_X"].reshape(-1, 3))[0]
        assert (np.abs(r).sum(1) > huber).mean() > 0.02
    p.close()


def _thresholds(pr, huber, kind):
    """Thresholds from a free 40-iteration run of the restatement, so that the
    stop rule really fires.  On these scenes every block stays clipped, so the
    step measure is the constant (0.02 + ~1e-3 (N + M)) / (N + M): the step rule
    fires on the first iteration with a threshold just above it.  The cost rule
    fires part-way with a threshold between the cost changes of the run."""
    free = gd_ref.solve(pr, max_iter=40, thr_step=0.0, thr_cost=0.0, huber=huber)
    cc = np.array([r["cost_change"] for r in free["rows"]])
    st = np.array([r["abs_step"] for r in free["rows"]])
    if kind in ("hover_fixed", "stereo", "w20"):
        return float(np.float32(st[0] * (1 + 1e-4))), 0.0, "step"
    return 0.0, float(np.float32(0.5 * (cc[5:30].min() + cc[5:30].max()))), "cost"


def _compare_run(rows, conv, p, ref, tol=1e-9, par=1e-8):
    rr = ref["rows"]
    decisive = min(r["margin"] for r in rr) > 1e-6
    if decisive:
        assert len(rows) == len(rr) and conv == ref["converged"]
    for g, r in zip(rows, rr):
        for f in ("cost", "abs_step", "average_reprojection_error"):
            assert abs(getattr(g, f) - r[f]) <= tol * abs(r[f]), f
        assert g.damping_term == r["damping_term"]
        assert g.abs_gradient == 0.0 and g.iteration_status == 0
        assert g.rho == 0.0 and g.model_change == 0.0 and g.trial_cost == g.cost
    if decisive:
        assert np.abs(p.get_poses() - ref["T_jw12"]).max() < par
        assert np.abs(p.get_points()[0] - ref["X"]).max() < par
    return decisive


@pytest.mark.parametrize("kind", KINDS)
def test_trajectory_matches_restatement(kind, built):
    sc, huber = scene(kind)
    pr = scenes.scaled_problem(sc)
    thr_step, thr_cost, rule = _thresholds(pr, huber, kind)
    ref = gd_ref.solve(pr, max_iter=40, thr_step=thr_step, thr_cost=thr_cost, huber=huber)
    p = make_gpu(pr)
    rows, conv = p.solve_gd(make_options(max_iter=40, thr_step=thr_step, thr_cost=thr_cost,
                                         huber=huber))
    assert _compare_run(rows, conv, p, ref)
    assert conv and len(rows) < 40          # the stop rule fired ...
    last = rows[-1]                         # ... the intended one
    assert (last.abs_step < thr_step) if rule == "step" else (last.cost_change < thr_cost)
    if rule == "cost":
        assert len(rows) > 1
    p.close()


def test_stop_rules_last_iteration_and_zero_iterations(built):
    sc, _ = scene("stereo")
    pr = scenes.scaled_problem(sc)
    p = make_gpu(pr)
    # threshold beyond every step: converged at once ... unless it is the last iteration
    rows, conv = p.solve_gd(make_options(max_iter=3, thr_step=1.0, thr_cost=0.0))
    assert len(rows) == 1 and conv
    p.update_values(pr["pose_T"], pr["pt_X"])
    rows, conv = p.solve_gd(make_options(max_iter=1, thr_step=1.0, thr_cost=0.0))
    assert len(rows) == 1 and not conv
    # max_num_iterations = 0: no row, not converged, parameters untouched
    p.update_values(pr["pose_T"], pr["pt_X"])
    rows, conv = p.solve_gd(make_options(max_iter=0))
    assert rows == [] and not conv
    assert (p.get_poses() == pr["pose_T"]).all() and (p.get_points()[0] == pr["pt_X"]).all()
    p.close()


def _bits(rows):
    return [(r.cost, r.cost_change, r.average_reprojection_error, r.abs_step,
             r.damping_term, r.iteration_status) for r in rows]


def test_deterministic_and_batch_independent(built):
    sc, _ = scene("masked")
    pr = scenes.scaled_problem(sc)
    out = []
    for _ in range(2):
        p = make_gpu(pr)
        rows, conv = p.solve_gd(make_options(max_iter=12, thr_step=0, thr_cost=0))
        out.append((_bits(rows), p.get_poses(), p.get_points()[0], p.gd_gradient()))
        p.close()
    assert out[0][0] == out[1][0]
    for k in (1, 2):
        assert (out[0][k] == out[1][k]).all()
    assert (out[0][3][0] == out[1][3][0]).all() and (out[0][3][1] == out[1][3][1]).all()
    # one batch of k iterations == k batches of one
    res = []
    for batches in ([12], [1] * 12):
        p = make_gpu(pr)
        p.gd_begin(make_options(max_iter=12, thr_step=0, thr_cost=0))
        for n in batches:
            p.gd_iterate(n)
        rows, n_it, conv, done = p.gd_sync(cap=12)
        assert done and n_it == 12
        res.append((_bits(rows), p.get_poses(), p.get_points()[0]))
        p.close()
    assert res[0][0] == res[1][0] == out[0][0]
    assert (res[0][1] == res[1][1]).all() and (res[0][2] == res[1][2]).all()


def test_lm_after_gd_equals_lm_on_a_fresh_handle(built):
    from oracle import oracle_py as O
    sc, _ = scene("stereo")
    pr = scenes.scaled_problem(sc)
    lm_opt = dict(max_iter=6, thr_step=0.0, thr_cost=0.0)
    # an LM solve on a handle that never ran GD: the rows of the oracle
    p0 = make_gpu(pr)
    rows0, _ = p0.solve(make_options(**lm_opt))
    orows, _ = O.Oracle(pr).solve(O.make_options(**lm_opt))
    assert len(rows0) == len(orows)
    for a, b in zip(rows0, orows):
        assert a.iteration_status == b.iteration_status
        assert abs(a.trial_cost - b.trial_cost) <= 1e-8 * abs(b.trial_cost)
    p0.close()
    # GD then LM on one handle == LM on a fresh handle seeded with the GD result
    p = make_gpu(pr)
    p.solve_gd(make_options(max_iter=10, thr_step=0, thr_cost=0))
    T, X = p.get_poses(), p.get_points()[0]
    rows_a, conv_a = p.solve(make_options(**lm_opt))
    q = make_gpu(pr)
    q.update_values(T, X)
    rows_b, conv_b = q.solve(make_options(**lm_opt))
    assert _bits(rows_a) == _bits(rows_b) and conv_a == conv_b
    assert [r.rho for r in rows_a] == [r.rho for r in rows_b]
    assert (p.get_poses() == q.get_poses()).all()
    assert (p.get_points()[0] == q.get_points()[0]).all()
    p.close()
    q.close()


def test_refusals(built):
    sc, _ = scene("hover_fixed")
    pr = scenes.scaled_problem(sc)
    s = make_gpu(pr, rank=0, world=2)
    with pytest.raises(BaError, match="sharded"):
        s.gd_begin(make_options())
    with pytest.raises(BaError, match="sharded"):
        s.solve_gd(make_options())
    s.close()
    p = make_gpu(pr)
    p.gd_begin(make_options())
    with pytest.raises(BaError, match="gradient-descent loop"):
        p.lm_iterate(1)
    p.lm_begin(make_options())
    with pytest.raises(BaError, match="LM loop"):
        p.gd_iterate(1)
    p.close()


def _mirror_solver(sc, fixed_pts):
    from bundle_adjustment_solver_amd import Camera, FullBundleAdjustmentSolverRefactor
    s = FullBundleAdjustmentSolverRefactor()
    for c in range(sc["intr"].shape[0]):
        s.RegisterCamera(c, Camera(*sc["intr"][c], pose_this_to_cam0=sc["T_cj"][c]))
    poses = [sc["T_wc_init"][k].copy() for k in range(len(sc["T_wc_init"]))]
    pts = [sc["X_init"][k].copy() for k in range(len(sc["X_init"]))]
    for T in poses:
        s.RegisterWorldToBodyPose(T)
    for X in pts:
        s.RegisterWorldPoint(X)
    for k in np.nonzero(sc["pose_fixed"])[0]:
        s.MakePoseFixed(poses[k])
    for k in fixed_pts:
        s.MakePointFixed(pts[k])
    for c, j, i, uv in zip(sc["obs_cam"], sc["obs_pose"], sc["obs_pt"], sc["obs_uv"]):
        s.AddObservation(int(c), poses[j], pts[i], uv)
    return s, poses, pts


def _options(max_iter, thr_step=1e-5, thr_cost=1e-5):
    from bundle_adjustment_solver_amd import Options
    opt = Options()
    opt.iteration_handle.max_num_iterations = max_iter
    opt.convergence_handle.threshold_step_size = thr_step
    opt.convergence_handle.threshold_cost_change = thr_cost
    return opt


def test_mirror_writes_back_and_fills_summary(built):
    from bundle_adjustment_solver_amd import Summary
    sc, _ = scene("hover_fixed")
    sc["pt_fixed"] = np.zeros(len(sc["X_init"]), bool)   # fixed points go through MakePointFixed
    fixed_pts = list(range(40))
    s, poses, pts = _mirror_solver(sc, fixed_pts)
    before_p = [T.copy() for T in poses]
    before_x = [X.copy() for X in pts]
    summ = Summary()
    assert s.SolveByGradientDescent(_options(25, 0.0, 0.0), summ)
    # the same problem through the ABI
    sc2 = dict(sc)
    sc2["pt_fixed"] = np.arange(len(sc["X_init"])) < 40
    pr = scenes.scaled_problem(sc2)
    p = make_gpu(pr)
    rows, conv = p.solve_gd(make_options(max_iter=25, thr_step=0.0, thr_cost=0.0))
    info = summ.optimization_info_list_
    assert len(info) == len(rows) == 25
    # (the mirror scales and inverts the user's poses itself: inputs equal up to roundoff)
    for i, r in zip(info, rows):
        for f in ("cost", "abs_step", "average_reprojection_error", "cost_change"):
            assert abs(getattr(i, f) - getattr(r, f)) <= 1e-9 * abs(getattr(r, f)), f
        assert i.damping_term == r.damping_term and int(i.iteration_status) == 0
    assert summ.convergence_status_ == conv
    for k in np.nonzero(sc["pose_fixed"])[0]:
        assert (poses[k] == before_p[k]).all()
    for k in fixed_pts:
        assert (pts[k] == before_x[k]).all()
    moved = [k for k in range(len(poses)) if not sc["pose_fixed"][k]]
    assert max(np.abs(poses[k] - before_p[k]).max() for k in moved) > 0
    X_abi = p.get_points()[0] * 100.0
    assert max(np.abs(pts[k] - X_abi[k]).max() for k in range(40, len(pts))) < 1e-10
    p.close()
    # max_num_iterations = 0: no rows, not converged, objects (up to the scaling round trip) unchanged
    s0, poses0, pts0 = _mirror_solver(sc, fixed_pts)
    ref_p = [T.copy() for T in poses0]
    ref_x = [X.copy() for X in pts0]
    summ0 = Summary()
    assert s0.SolveByGradientDescent(_options(0), summ0)
    assert summ0.optimization_info_list_ == [] and summ0.convergence_status_ is False
    for a, b in zip(poses0, ref_p):
        assert np.abs(a - b).max() < 1e-12
    for a, b in zip(pts0, ref_x):
        assert np.abs(a - b).max() < 1e-12


def test_cpp_facade_matches_python_mirror(tmp_path, built):
    from bundle_adjustment_solver_amd import Summary
    sc = scenes.synthetic_ba_scene(12, 400, 5, True, seed=71)
    fixed_pts = list(range(10))
    sc["pt_fixed"] = np.zeros(len(sc["X_init"]), bool)
    n_cam, n_pose, n_pt, n_obs = (len(sc["intr"]), len(sc["T_wc_init"]), len(sc["X_init"]),
                                  len(sc["obs_uv"]))
    f12 = lambda T: " ".join("%.17e" % v for v in list(T[:3, :3].ravel()) + list(T[:3, 3]))
    lines = ["%d %d %d %d" % (n_cam, n_pose, n_pt, n_obs)]
    for c in range(n_cam):
        lines.append(" ".join("%.17e" % v for v in sc["intr"][c]) + " " + f12(sc["T_cj"][c]))
    for j in range(n_pose):
        lines.append("%d %s" % (int(sc["pose_fixed"][j]), f12(sc["T_wc_init"][j])))
    for i in range(n_pt):
        lines.append("%d %s" % (int(i in fixed_pts), " ".join("%.17e" % v for v in sc["X_init"][i])))
    for c, j, i, uv in zip(sc["obs_cam"], sc["obs_pose"], sc["obs_pt"], sc["obs_uv"]):
        lines.append("%d %d %d %.17e %.17e" % (c, j, i, uv[0], uv[1]))
    lines.append("30 0 0.0001 1 100")
    path = tmp_path / "gd_problem.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([os.path.join(ROOT, "cpp", "build", "test_gd"), str(path)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "GD FACADE TEST PASSED" in r.stdout, r.stdout[-3000:]
    rows = [list(map(float, l.split()[1:])) for l in r.stdout.splitlines() if l.startswith("row ")]
    cposes = np.array([list(map(float, l.split()[1:])) for l in r.stdout.splitlines()
                       if l.startswith("pose ")]).reshape(-1, 3, 4)
    cpts = np.array([list(map(float, l.split()[1:])) for l in r.stdout.splitlines()
                     if l.startswith("point ")])
    conv = int([l for l in r.stdout.splitlines() if l.startswith("converged")][0].split()[1])
    s, poses, pts = _mirror_solver(sc, fixed_pts)
    summ = Summary()
    s.SolveByGradientDescent(_options(30, 0.0, 1e-4), summ)
    info = summ.optimization_info_list_
    assert len(info) == len(rows) > 0 and conv == int(summ.convergence_status_)
    for i, row in zip(info, rows):
        got = [i.cost, i.cost_change, i.average_reprojection_error, i.abs_step, i.abs_gradient,
               i.damping_term]
        assert np.allclose(row[:6], got, rtol=1e-12, atol=0)
        assert int(row[6]) == int(i.iteration_status)
    assert np.abs(cposes - np.array([T[:3, :4] for T in poses])).max() < 1e-12
    assert np.abs(cpts - np.array(pts)).max() < 1e-12
