"""GPU tests of the relative-pose factors on the handle path (ba_set_relative,
BaProblem.set_relative, AddRelativePose; csrc/ba_rel.hip).

Reference: rel_ref.lm_with_relatives / dense_factors / cov_with_relatives on the CPU oracle,
used as they are.  The scenes, the factor set and the pins that make the comparison
meaningful (the reference accepts and rejects, no gain ratio near a threshold, the factors
move the first trial cost) are in rel_handle_cases.py / test_rel_handle_ref.py.

Tolerances are the project's: iteration_status identical, damping_term 1e-12, cost and trial
cost 1e-7 relative (assert_same_trajectory), final parameters RTOL_FINAL on the north-star
metrics, S and rhs 1e-9 relative as test_gpu_parity uses for get_S.
"""
import numpy as np
import pytest

from bundle_adjustment_solver_amd._lib import BaError, make_options
from bundle_adjustment_solver_amd.solver import (BaBatch, BaProblem, Camera, FullBundleAdjustmentSolver,
                                                 FullBundleAdjustmentSolverRefactor)
from bundle_adjustment_solver_amd import scenes
from oracle import oracle_py as O

import rel_cases
import rel_handle_cases as cases
import rel_ref
from cov_ref import rel_block_diff
from test_gpu_parity import RTOL_FINAL, assert_same_trajectory, make_gpu, pose_errors, relerr

pytestmark = pytest.mark.gpu


def make_rel(pr, rels, finalize=True):
    p = BaProblem(0)
    p.set_cameras(pr["cam_intr"], pr["cam_T"])
    p.set_poses(pr["pose_T"], pr["pose_fixed"])
    p.set_points(pr["pt_X"], pr["pt_fixed"])
    p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
    if rels is not None:
        p.set_relative(rels)
    if finalize:
        p.finalize()
    return p


def final_errors(g, ref):
    """the north-star metrics between the handle's parameters and the reference's"""
    _, _, oT, oX = ref
    ang, dt = pose_errors(g.get_poses(), oT)
    X = g.get_points()[0]
    dX = (np.linalg.norm(X - oX, axis=1) / np.maximum(np.linalg.norm(oX, axis=1), 1e-300)).max()
    return ang, dt, dX


def check_against_reference(name, g, rows, ref):
    for k, (a, b) in enumerate(zip(rows, ref[0])):
        print("%s it %d: status %d/%d lambda %.6g/%.6g trial cost %.12g/%.12g rho %.4g/%.4g"
              % (name, k, a.iteration_status, b.iteration_status, a.damping_term, b.damping_term,
                 a.trial_cost, b.trial_cost, a.rho, b.rho))
    assert_same_trajectory(rows, ref[0])
    errs = final_errors(g, ref)
    print(name, "final errors", errs)
    assert max(errs) <= RTOL_FINAL, errs


# ---- 1. blocks ----------------------------------------------------------------------------------
def test_blocks_match_the_oracle_plus_the_dense_factors(built):
    pr, rels = cases.case("small30")
    lam, hub = 0.5, 1.0
    g = make_rel(pr, rels)
    o = O.Oracle(pr)
    o.linearize(hub)
    o.damp_invert(lam)
    o.schur()
    g.stage_linearize(lam, hub)
    g.stage_schur()
    S, rhs = g.get_S()
    oS, orhs = o.get_S()
    H, gr = rel_ref.dense_factors(pr, o.get_poses(), rels)
    Hd = H + lam * np.diag(np.diag(H))
    print("S", relerr(S, oS + Hd), "rhs", relerr(rhs, orhs + gr), "factors alone", relerr(S, oS))
    assert relerr(S, oS + Hd) < 1e-9 and relerr(rhs, orhs + gr) < 1e-9
    assert relerr(S, oS) > 1e-3   # the factors are felt
    A, a = g.get_A()
    oA, oa = o.get_A()
    N = g.N
    Hjj = np.stack([Hd[6 * j:6 * j + 6, 6 * j:6 * j + 6] for j in range(N)])
    assert relerr(A, oA + Hjj) < 1e-9 and relerr(a, oa + gr.reshape(N, 6)) < 1e-9
    assert np.array_equal(A, A.transpose(0, 2, 1))
    want = o.cost() + rel_ref.rel_norm(o.get_poses(), rels)
    assert relerr(g.stage_cost(), want) < 1e-12
    info = g.relative_info()
    print(info)
    assert info["factors"] == rel_ref.n_factors(rels) and info["blocks_only"] >= 1
    assert info["blocks"] > info["blocks_only"] and info["bytes"] > 0
    o.close()
    g.close()


# ---- 2. trajectory, group path -------------------------------------------------------------------
def test_trajectory_on_the_group_path(built):
    pr, rels = cases.case("group150")
    g = make_rel(pr, rels)
    li = g.get_lin_info()
    assert li["pose_major_observations"] == 0 and li["chunks"] == 0
    rows, _ = g.solve(make_options(**cases.LM))
    check_against_reference("group150", g, rows, cases.reference("group150"))
    assert g.get_dropped_pivots() == 0
    plain = make_gpu(pr)
    print("dense info", g.get_dense_info(), plain.get_dense_info())
    assert g.get_dense_info() != plain.get_dense_info()   # the far pairs couple tiles that no landmark couples
    plain.close()
    g.close()


# ---- 3. trajectory, chunk path -------------------------------------------------------------------
@pytest.mark.parametrize("gn", [False, True])
def test_trajectory_on_the_chunk_path(built, gn):
    pr, rels = cases.case("chunk60")
    g = make_rel(pr, rels)
    assert g.get_schur_info()["grouped_landmarks"] < 0.2 * g.M_global
    rows, _ = g.solve(make_options(**(cases.GN if gn else cases.LM)))
    check_against_reference("chunk60 gn=%d" % gn, g, rows, cases.reference("chunk60", gn))
    assert g.get_dropped_pivots() == 0
    g.close()


# ---- 4. a pose held by factors only --------------------------------------------------------------
def test_a_pose_without_observations_is_held_by_its_factors(built):
    pr, rels = cases.case("blind30")
    g = make_rel(pr, rels)
    rows, _ = g.solve(make_options(**cases.LM))
    check_against_reference("blind30", g, rows, cases.reference("blind30"))
    assert g.get_dropped_pivots() == 0
    g.close()
    plain = make_gpu(pr)
    plain.solve(make_options(**cases.LM))
    assert plain.get_dropped_pivots() > 0
    plain.close()


# ---- 5. against the batch path -------------------------------------------------------------------
def test_handle_and_batch_agree(built):
    for name, _, pr, rels in rel_cases.parity_cases():
        b = BaBatch([pr])
        b.set_relative([rels])
        brows, res = b.solve(make_options(**rel_cases.FIXED))
        bT, bX = b.poses_of(0, b.get_poses()).copy(), b.points_of(0, b.get_points()).copy()
        b.close()
        g = make_rel(pr, rels)
        rows, _ = g.solve(make_options(**rel_cases.FIXED))
        assert res[0].status == 0
        assert_same_trajectory(rows, brows[0])
        errs = final_errors(g, (None, None, bT, bX))
        print(name, errs)
        assert max(errs) <= RTOL_FINAL
        g.close()


# ---- 6. bits -------------------------------------------------------------------------------------
def run(g, T0, X0, opt=None):
    g.update_values(T0, X0)
    rows, _ = g.solve(make_options(**(opt or cases.LM)))
    return ([(r.iteration_status, r.trial_cost, r.damping_term, r.cost) for r in rows], g.get_poses().copy(),
            g.get_points()[0].copy())


def same_bits(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_bits(built):
    pr, rels = cases.case("small30")
    T0, X0 = pr["pose_T"], pr["pt_X"]
    g = make_rel(pr, rels)
    first = run(g, T0, X0)
    assert same_bits(run(g, T0, X0), first)                  # run to run
    g.update_relative(rels["Z"], rels["Omega"])
    assert same_bits(run(g, T0, X0), first)                  # the same values again
    # a refused update changes nothing
    bad = rels["Z"].copy()
    bad[3, 4] = np.nan
    with pytest.raises(BaError, match="factor 3"):
        g.update_relative(bad, rels["Omega"])
    assert same_bits(run(g, T0, X0), first)
    moved = rels["Z"].copy()
    moved[:, 9:] += 1e-3
    g.update_relative(moved, rels["Omega"])
    assert run(g, T0, X0)[0][0][1] != first[0][0][1]         # the first trial cost moves
    g.close()
    # set, clear, finalize: the handle that never had factors
    plain = make_gpu(pr)
    ref = run(plain, T0, X0)
    plain.close()
    c = make_rel(pr, rels, finalize=False)
    c.set_relative(None)
    c.finalize()
    assert c.relative_info()["factors"] == 0
    assert same_bits(run(c, T0, X0), ref)
    c.close()
    assert not same_bits(first, ref)
    # a refused set_relative leaves the factors set before it
    d = make_rel(pr, rels, finalize=False)
    wrong = dict(rels, k=rels["j"].copy())
    with pytest.raises(BaError, match="j == k"):
        d.set_relative(wrong)
    d.finalize()
    assert same_bits(run(d, T0, X0), first)
    d.close()


# ---- 7. refusals on a live handle ----------------------------------------------------------------
def test_refusals_leave_a_working_handle(built):
    pr, rels = cases.case("small30")
    opt = dict(cases.LM, max_iter=2)
    g = make_rel(pr, rels, finalize=False)
    with pytest.raises(BaError, match="one GPU"):
        g.set_shard(0, 2)                                    # factors, then shard
    g.finalize()
    with pytest.raises(BaError, match="relative-pose factors"):
        g.solve_gd(make_options(**opt))
    with pytest.raises(BaError, match="already finalized"):
        g.set_relative(rels)
    want = [r.trial_cost for r in cases.reference("small30")[0][:2]]
    rows, _ = g.solve(make_options(**opt))
    assert len(rows) == 2 and relerr([r.trial_cost for r in rows], want) < 1e-7
    g.close()
    s = make_rel(pr, None, finalize=False)
    s.set_shard(0, 2)
    with pytest.raises(BaError, match="one GPU"):
        s.set_relative(rels)                                 # shard, then factors
    s.close()


def test_graph_replay_is_refused_with_factors(built, monkeypatch):
    """BA_GRAPH=1 (read once, by ba_create): the captured iteration was not extended to the
    factor launches, so such a handle refuses the factors and solves without them"""
    pr, rels = cases.case("small30")
    monkeypatch.setenv("BA_GRAPH", "1")
    g = make_rel(pr, None, finalize=False)
    monkeypatch.delenv("BA_GRAPH")
    with pytest.raises(BaError, match="BA_GRAPH"):
        g.set_relative(rels)
    g.finalize()
    rows, _ = g.solve(make_options(**dict(cases.LM, max_iter=2)))
    want = [r.trial_cost for r in cases.plain_oracle_rows("small30")[:2]]
    assert g.relative_info()["factors"] == 0 and relerr([r.trial_cost for r in rows], want) < 1e-7
    g.close()


# ---- 8. covariance -------------------------------------------------------------------------------
def test_covariance_includes_the_factors(built):
    pr, rels = cases.case("small30")
    cp, cq, noise = rel_ref.cov_with_relatives(pr, rels)
    assert noise <= 1e-8, "scene unfit: the two host references disagree"
    ps = np.flatnonzero(np.asarray(pr["pose_fixed"]) == 0)
    qs = np.flatnonzero(np.asarray(pr["pt_fixed"]) == 0)
    g = make_rel(pr, rels)
    gp, gq, dropped = g.covariance(ps, qs, 1.0)
    g.close()
    plain = make_gpu(pr)
    fp, _, _ = plain.covariance(ps, qs, 1.0)
    plain.close()
    err_p, err_q = rel_block_diff(gp, cp[ps]), rel_block_diff(gq, cq[qs])
    tol = 10.0 * max(noise, 1e-12)
    print("noise %.3e pose %.3e point %.3e, without factors %.3e" % (noise, err_p, err_q, rel_block_diff(fp, cp[ps])))
    assert dropped == 0 and err_p <= tol and err_q <= tol
    assert rel_block_diff(fp, cp[ps]) > 1e-3


# ---- 9. facade -----------------------------------------------------------------------------------
def facade(cls, sc, pairs, sigma):
    s = cls(0)
    for c in range(sc["intr"].shape[0]):
        s.AddCamera(c, Camera(*sc["intr"][c], pose_this_to_cam0=sc["T_cj"][c]))
    poses, pts = sc["T_wc_init"].copy(), sc["X_init"].copy()
    hp, hq = s.AddPoseArray(poses), s.AddPointArray(pts)
    for j in np.nonzero(sc["pose_fixed"])[0]:
        s.MakePoseFixed(int(hp[j]))
    for c in range(sc["intr"].shape[0]):
        m = sc["obs_cam"] == c
        s.AddObservations(c, hp[sc["obs_pose"][m]], hq[sc["obs_pt"][m]], sc["obs_uv"][m])
    rng = np.random.default_rng(3)
    facs = []
    for j, k in pairs:
        J = rng.standard_normal((8, 6)) * 30.0
        M = np.linalg.inv(sc["T_wc_true"][j]) @ sc["T_wc_true"][k]
        facs.append(dict(pose_j=int(hp[j]), pose_k=int(hp[k]), measurement=M, information=J.T @ J))
    for f in facs:
        s.AddRelativePose(f["pose_j"], f["pose_k"], f["measurement"], f["information"], sigma_pixel=sigma)
    return s, facs, poses, pts


@pytest.mark.parametrize("cls", [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor])
def test_facade_is_the_raw_call_on_the_scaled_arrays(built, cls):
    sc = scenes.synthetic_ba_scene(12, 150, 5, True, seed=12)
    nf = int(np.asarray(sc["pose_fixed"]).sum())
    pairs = [(q + 1, q) for q in range(nf - 1, 11)] + [(11, nf + 1), (nf, 9)]
    sigma = 0.7
    s, facs, poses, pts = facade(cls, sc, pairs, sigma)
    s.FinalizeParameters()
    sr = FullBundleAdjustmentSolver._scaled_relatives("test", [s], [facs], sigma)[0]
    intr, camT, T_jw, X, pf, qf, ocam, opose, opt_, ouv = s._host_arrays()
    pr = dict(cam_intr=intr, cam_T=camT, pose_T=T_jw, pose_fixed=pf, pt_X=X, pt_fixed=qf, obs_cam=ocam,
              obs_pose=opose, obs_pt=opt_, obs_uv=ouv)
    g = make_rel(pr, sr)
    assert s._problem.relative_info() == g.relative_info() and g.relative_info()["factors"] == len(pairs)
    opt = make_options(max_iter=4, thr_step=0.0, thr_cost=0.0)
    rows, _ = g.solve(opt)
    frows, _ = s._problem.solve(opt)
    assert [(r.trial_cost, r.iteration_status) for r in rows] == [(r.trial_cost, r.iteration_status) for r in frows]
    assert np.array_equal(g.get_poses(), s._problem.get_poses())
    # after FinalizeParameters the call warns and is ignored; ReloadParameterValues keeps the
    # factors, Reset drops them
    s.AddRelativePose(facs[0]["pose_j"], facs[0]["pose_k"], facs[0]["measurement"], facs[0]["information"])
    assert len(s._relatives) == len(pairs)
    s.ReloadParameterValues()
    assert s._problem.relative_info()["factors"] == len(pairs)
    s.Reset()
    assert s._relatives == []
    g.close()
