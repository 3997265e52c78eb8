"""GPU tests of the robust kernels of the pose-graph optimisation (ba_pgraph_set_robust,
ba_pgraph_factor_report, BaPoseGraph.set_robust, AddRelativePose(robust=...); k_pg_lin_robust and
k_pg_assemble_robust of csrc/ba_pgraph.hip).

Reference: pgo_robust_ref (numpy fp64: pgo_ref.lm with sum rho for chi-square and w Omega for
Omega) on the seeded scenes of pgo_robust_cases.py, whose fitness for a trajectory comparison
test_pgo_robust_ref.py pins without a GPU.

Sizes: 1, 5, 6, 10, 11 and 59 optimisable poses; 63 / 64 / 65 factors around one k_pg_lin
workgroup of 64 with the robust factor on either side of the edge; 329 poses for several
workgroups and levels.

Tolerances, those of test_gpu_pose_graph.py: H and g 1e-9 relative, the cost 1e-12 relative, s
and w of the report 1e-12 relative; trajectories: status identical, lambda 1e-12, cost and trial
cost 1e-7 relative; final poses max_j |se3_log(T_gpu T_ref^-1)| <= 10 max(noise, 1e-12) with noise
the distance between the numpy-solve and the Cholesky-solve runs of the reference, the scene
unfit if noise > 1e-8.
"""
import numpy as np
import pytest

from bundle_adjustment_solver_amd._lib import BaError, make_options
from bundle_adjustment_solver_amd.solver import (ROBUST_CAUCHY, ROBUST_GEMAN_MCCLURE, ROBUST_HUBER, SCALER, BaPoseGraph,
                                                 FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor,
                                                 Options, Summary, _T12_to_44, rigid_inverse)

import pgo_cases
import pgo_ref
import pgo_robust_cases as cases
import pgo_robust_ref as ref
import rel_ref
from prior_ref import sym_lower
from test_gpu_pose_graph import assert_same_trajectory, relerr, row_bits

pytestmark = pytest.mark.gpu


def make(g, kernels=True):
    p = BaPoseGraph(g["pose_T"], g["pose_fixed"], g["rels"])
    if kernels:
        p.set_robust(g["kind"], g["scale"])
    return p


def check_system(g, tag=""):
    """weighted system, cost and factor report at the start poses against the reference"""
    p = make(g)
    H, gr = p.system()
    rH, rg = ref.system(g, g["pose_T"])
    c, rc = p.cost(), ref.cost(g["pose_T"], g)
    s, w = p.factor_report()
    rs, rw = ref.report(g["pose_T"], g)
    es, ew = np.abs(s - rs) / rs, np.abs(w - rw) / rw
    print(tag, "H", relerr(H, rH), "g", relerr(gr, rg), "cost", abs(c - rc) / rc, "s", es.max(), "w", ew.max(),
          "weights in [%.3g, %.3g]" % (w.min(), w.max()))
    assert relerr(H, rH) < 1e-9 and relerr(gr, rg) < 1e-9
    assert np.array_equal(H, H.T)
    assert abs(c - rc) <= 1e-12 * rc
    assert es.max() <= 1e-12 and ew.max() <= 1e-12
    assert np.array_equal(p.poses(), g["pose_T"])   # none of the calls moves the poses
    p.close()
    return w


def check_trajectory(name, p):
    ref_rows, ref_conv, ref_T = cases.reference(name)
    rows, conv = p.solve(cases.options(name))
    for k, (a, b) in enumerate(zip(rows, ref_rows)):
        print("%s it %d: status %d/%d lambda %.6g/%.6g trial %.12g/%.12g cost %.12g/%.12g rho %.4g/%.4g"
              % (name, k, a.iteration_status, b.iteration_status, a.damping_term, b.damping_term,
                 a.trial_cost, b.trial_cost, a.cost, b.cost, a.rho, b.rho))
    assert_same_trajectory(rows, ref_rows)
    assert conv == ref_conv
    noise = pgo_ref.pose_distance(cases.reference_cholesky(name)[2], ref_T)
    assert noise <= 1e-8, "scene unfit: the two host references disagree"
    err = pgo_ref.pose_distance(p.poses(), ref_T)
    print("%s final poses: error %.3e, noise of the host reference %.3e, pivots %d"
          % (name, err, noise, p.info()["bad_pivots"]))
    assert err <= 10.0 * max(noise, 1e-12)
    assert p.info()["bad_pivots"] == 0
    return 10.0 * max(noise, 1e-12)


def report_bounds(g, rs, E):
    """How far s and w may lie from the reference's when every pose lies within E of the
    reference's pose (the rule above).  A tangent step eps of T_j moves r = log(T_j T_k^-1 Z^-1)
    by eps to first order, one of T_k by Ad(T_j T_k^-1) eps, whose norm is at most (1 + |t_E|)
    |eps|; with |t_E| <= 2 max |t| and a factor 2 for the second order, |dr| <= d = 4 E (1 + 2 max
    |t|).  Then |ds| <= 2 sqrt(s lmax) d + lmax d^2 with lmax the largest eigenvalue of Omega,
    and |dw| <= 2 |ds| / c^2: |w'| <= 1 / c^2 (Cauchy), 2 / c^2 (Geman-McClure), 1 / (2 c^2)
    (Huber beyond the knee).  1e-12 relative is added for the arithmetic itself."""
    d = 4.0 * E * (1.0 + 2.0 * np.abs(np.asarray(g["pose_T"])[:, 9:]).max())
    lmax = np.array([np.linalg.eigvalsh(sym_lower(o)).max() for o in np.asarray(g["rels"]["Omega"]).reshape(-1, 6, 6)])
    ds = 2.0 * np.sqrt(rs * lmax) * d + lmax * d * d + 1e-12 * rs
    return ds, 2.0 * ds / np.asarray(g["scale"], np.float64) ** 2 + 1e-12


# ---- 1. system, cost and report -----------------------------------------------------------------
@pytest.mark.parametrize("kind", [ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_GEMAN_MCCLURE])
def test_each_kind_alone(built, kind):
    w = check_system(cases.with_kernels(pgo_cases.scene("g60"), kind, "all"), "kind %d" % kind)
    assert w.min() < 0.5   # the kernel bites


@pytest.mark.parametrize("name", ["g2", "g12", "g60", "g330"])
def test_all_kinds_mixed_inside_one_workgroup(built, name):
    g = cases.with_kernels(cases.corrupt(pgo_cases.scene(name), 1), 0, "mixed")
    assert name in ("g2", "g12") or set(g["kind"][:64].tolist()) == {0, 1, 2, 3}
    w = check_system(g, name)
    assert np.all(w[g["kind"] == 0] == 1.0)


# ---- 2. the workgroup edge ----------------------------------------------------------------------
@pytest.mark.parametrize("name,f", [("g60_63", 62), ("g60", 63), ("g60_65", 63), ("g60_65", 64)])
@pytest.mark.parametrize("kind", [ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_GEMAN_MCCLURE])
def test_robust_factor_at_the_workgroup_edge(built, name, f, kind):
    """63, 64 and 65 factors: the one robust factor is the last of the first k_pg_lin workgroup
    (the last factor of a partial one for 63), then the first of the second"""
    g = pgo_cases.scene(name)
    assert len(g["rels"]["j"]) == dict(g60_63=63, g60=64, g60_65=65)[name]
    w = check_system(cases.with_kernels(g, kind, [f], scale=1.0), "%s factor %d" % (name, f))
    assert w[f] < 0.5 and np.all(np.delete(w, f) == 1.0)


# ---- 3. fixed ends, twins, small graphs ---------------------------------------------------------
def test_fixed_ends_and_twins(built):
    g = pgo_cases.scene("g60")
    j, k, fx = g["rels"]["j"], g["rels"]["k"], g["pose_fixed"]
    k_fixed = int(np.flatnonzero((fx[k] != 0) & (fx[j] == 0))[0])
    j_fixed = int(np.flatnonzero((fx[j] != 0) & (fx[k] == 0))[0])
    for f in (k_fixed, j_fixed):
        w = check_system(cases.with_kernels(g, ROBUST_CAUCHY, [f], scale=1.0), "fixed end, factor %d" % f)
        assert w[f] < 0.5
    # a twin of a closure between two optimisable poses: the same pair the other way round
    f = int(np.flatnonzero((fx[j] == 0) & (fx[k] == 0) & (np.abs(j - k) > 1))[0])
    rels = dict(j=np.r_[j, k[f]].astype(np.int32), k=np.r_[k, j[f]].astype(np.int32),
                Z=np.vstack([g["rels"]["Z"], rel_ref.inverse12(g["rels"]["Z"][f])[None]]),
                Omega=np.concatenate([g["rels"]["Omega"], 0.5 * g["rels"]["Omega"][f:f + 1]]))
    twin = dict(g, rels=rels)
    F = len(rels["j"])
    for robust_one in (f, F - 1):   # one of the pair robust, the other not
        w = check_system(cases.with_kernels(twin, ROBUST_GEMAN_MCCLURE, [robust_one], scale=1.0),
                         "twin pair, robust factor %d" % robust_one)
        assert w[robust_one] < 0.5 and w[f if robust_one != f else F - 1] == 1.0


def test_two_pose_graph(built):
    g = cases.scene("r2")
    check_system(g, "r2")
    p = make(g)
    check_trajectory("r2", p)
    p.close()


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("name", ["rn5", "rn6", "rn10", "rn11"])
def test_pose_per_tile_edges(built, monkeypatch, name, nb):
    """N = 5, 6, 10, 11 optimisable poses: a full tile of 5 / 10 poses, one pose into the next"""
    monkeypatch.setenv("BA_DENSE_NB", str(nb))   # read by ba_create
    p = make(cases.scene(name))
    monkeypatch.delenv("BA_DENSE_NB")
    info = p.info()
    ppt = 5 if nb == 32 else 10
    assert info["N"] == int(name[2:]) and info["nb"] == nb and info["tiles"] == (info["N"] + ppt - 1) // ppt
    check_trajectory(name, p)
    p.close()


# ---- 4. s = 0 -----------------------------------------------------------------------------------
def test_zero_residuals_give_unit_weights(built):
    # every pose the identity, every Z the identity: r = 0 and s = 0 to the bit
    n = 9
    eye = np.r_[np.eye(3).reshape(9), np.zeros(3)]
    fx = np.zeros(n, np.uint8)
    fx[0] = 1
    j = np.arange(1, n, dtype=np.int32)
    rels = dict(j=j, k=j - 1, Z=np.tile(eye, (n - 1, 1)), Omega=pgo_cases.scene("g12")["rels"]["Omega"][:n - 1])
    g = cases.with_kernels(dict(pose_T=np.tile(eye, (n, 1)), pose_fixed=fx, rels=rels), 0, "mixed", scale=1e-3)
    p = make(g)
    s, w = p.factor_report()
    assert np.all(s == 0.0) and np.all(w == 1.0) and p.cost() == 0.0
    H, gr = p.system()
    assert np.isfinite(H).all() and np.all(gr == 0.0)
    p.close()
    # exact Z with the start at the truth: s is zero to rounding, every weight 1, and a solve
    # leaves nothing non-finite behind
    t = pgo_cases.scene("x12")
    g = cases.with_kernels(dict(t, pose_T=t["truth"].copy()), 0, "mixed", scale=1.0)
    p = make(g)
    s, w = p.factor_report()
    print("s at the truth: max %.3e" % s.max())
    assert s.max() <= 1e-18 and np.all(w == 1.0)   # 1 + 1e-18 is 1 in fp64
    rows, _ = p.solve(make_options(max_iter=3, **cases.LM))
    for r in rows:
        vals = [r.cost, r.trial_cost, r.cost_change, r.average_reprojection_error, r.abs_step, r.damping_term,
                r.rho, r.model_change]
        print("it: status %d" % r.iteration_status, vals)
        assert np.isfinite(vals).all()
    assert np.isfinite(p.poses()).all() and pgo_ref.pose_distance(p.poses(), t["truth"]) < 1e-9
    s, w = p.factor_report()
    assert np.all(np.abs(w - 1.0) <= 1e-12)
    p.close()


# ---- 5. trajectories ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["r40_huber", "r40_cauchy", "r40_gm", "r60_huber", "r60_mixed", "r60_cauchy",
                                  "r60_gm"])
def test_trajectory_matches_the_reference(built, name):
    p = make(cases.scene(name))
    E = check_trajectory(name, p)
    # the report after the solve is the reference's at its final poses, as far as poses within
    # E of the reference's allow
    g = cases.scene(name)
    s, w = p.factor_report()
    rs, rw = ref.report(cases.reference(name)[2], g)
    ds, dw = report_bounds(g, rs, E)
    print(name, "report after the solve: s off by at most %.3g of its bound, w by %.3g of its bound"
          % ((np.abs(s - rs) / ds).max(), (np.abs(w - rw) / dw).max()))
    assert (np.abs(s - rs) <= ds).all() and (np.abs(w - rw) <= dw).all()
    p.close()


# ---- 6. outliers, end to end --------------------------------------------------------------------
def test_false_closures_are_switched_off(built):
    name = "o40"
    g, bad, good = cases.outlier_scene(name)
    clean = cases.outlier_clean(name)
    opt = cases.outlier_options()
    p = make(g, kernels=False)
    p.solve(opt)
    d_none = pgo_ref.pose_distance(p.poses(), clean)
    s, w = p.factor_report()
    assert np.all(w == 1.0)
    # the same object, back at the start, with Geman-McClure on the closures
    gk = cases.with_kernels(g, ROBUST_GEMAN_MCCLURE, "closures")
    p.update_values(g["pose_T"])
    p.set_robust(gk["kind"], gk["scale"])
    rows, _ = p.solve(opt)
    T = p.poses()
    d_gm = pgo_ref.pose_distance(T, clean)
    s, w = p.factor_report()
    print("distance to the clean solution: none %.4g, Geman-McClure %.4g; largest outlier weight %.3g, smallest "
          "inlier-closure weight %.3g" % (d_none, d_gm, w[bad].max(), w[good].min()))
    assert d_none >= 1.0 and d_gm <= 0.02
    assert w[bad].max() < 1e-2 and w[good].min() > 0.8
    ref_T = cases.outlier_reference(name, ref.GM)[2]
    noise = pgo_ref.pose_distance(cases.outlier_reference(name, ref.GM, True)[2], ref_T)
    err = pgo_ref.pose_distance(T, ref_T)
    print("final poses: error %.3e, noise of the host reference %.3e" % (err, noise))
    assert noise <= 1e-8 and err <= 10.0 * max(noise, 1e-12)
    p.close()


# ---- 7. off is off ------------------------------------------------------------------------------
def test_no_kernel_is_the_plain_solver_to_the_bit(built):
    name = "g60"
    g = pgo_cases.scene(name)
    opt = pgo_cases.options(name)
    F = len(g["rels"]["j"])
    plain = make(g, kernels=False)
    r0, _ = plain.solve(opt)
    T0 = plain.poses()
    plain.close()
    for tag in ("zeros", "null", "after_robust"):
        p = make(g, kernels=False)
        if tag == "zeros":
            p.set_robust(np.zeros(F, np.int32), np.zeros(F))
        elif tag == "null":
            p.set_robust(None)
        else:   # kernels set, then cleared: the plain kernels again
            p.set_robust(np.full(F, ROBUST_CAUCHY, np.int32), np.full(F, 30.0))
            assert p.cost() < 0.5 * pgo_ref.chi2(g["pose_T"], g["rels"])
            p.set_robust(None)
        r, _ = p.solve(opt)
        assert row_bits(r) == row_bits(r0) and np.array_equal(p.poses(), T0), tag
        p.close()
    # Huber with c = 1e30 on every factor: w = 1 and rho = s through the robust kernels
    p = make(g, kernels=False)
    p.set_robust(np.full(F, ROBUST_HUBER, np.int32), np.full(F, 1e30))
    r, _ = p.solve(opt)
    same = row_bits(r) == row_bits(r0) and np.array_equal(p.poses(), T0)
    print("Huber with c = 1e30 against the plain kernels: the bits", "agree" if same else "differ")
    assert len(r) == len(r0)
    for a, b in zip(r, r0):
        assert a.iteration_status == b.iteration_status and a.damping_term == b.damping_term
        assert abs(a.cost - b.cost) <= 1e-12 * abs(b.cost) and abs(a.trial_cost - b.trial_cost) <= 1e-12 * abs(b.trial_cost)
    p.close()


# ---- 8. re-solves -------------------------------------------------------------------------------
def test_set_robust_between_solves(built):
    name = "r60_cauchy"
    g = cases.scene(name)
    opt = cases.options(name)
    fresh = make(g)
    r0, _ = fresh.solve(opt)
    T0 = fresh.poses()
    # the same object again from the start: the same bits
    fresh.update_values(g["pose_T"])
    r1, _ = fresh.solve(opt)
    assert row_bits(r1) == row_bits(r0) and np.array_equal(fresh.poses(), T0)
    fresh.close()
    # an object that solved without kernels first, then took them: equal to the fresh one
    p = make(g, kernels=False)
    p.solve(opt)
    p.update_values(g["pose_T"])
    p.set_robust(g["kind"], g["scale"])
    r2, _ = p.solve(opt)
    assert row_bits(r2) == row_bits(r0) and np.array_equal(p.poses(), T0)
    # another scale on the same object changes the result; update_values keeps the kernels
    p.set_robust(g["kind"], 0.25 * g["scale"])
    p.update_values(g["pose_T"])
    r3, _ = p.solve(opt)
    assert row_bits(r3) != row_bits(r0)
    q = make(dict(g, scale=0.25 * g["scale"]))
    r4, _ = q.solve(opt)
    assert row_bits(r3) == row_bits(r4) and np.array_equal(p.poses(), q.poses())
    # a refused call changes nothing
    bad = g["scale"].copy()
    bad[5] = -1.0
    with pytest.raises(BaError, match="factor 5"):
        p.set_robust(g["kind"], bad)
    p.update_values(g["pose_T"])
    r5, _ = p.solve(opt)
    assert row_bits(r5) == row_bits(r3)
    p.close()
    q.close()


# ---- 9. facades ---------------------------------------------------------------------------------
def pose_facade(cls, g, sigma):
    """the poses and factors of a graph on a facade object, in the caller's units; the robust
    scale goes in as a Mahalanobis distance of the caller's information"""
    s = cls(0)
    T44 = _T12_to_44(g["pose_T"])
    T44[:, :3, 3] /= SCALER
    poses = rigid_inverse(T44)
    hp = s.AddPoseArray(poses)
    for q in np.flatnonzero(g["pose_fixed"]):
        s.MakePoseFixed(int(hp[q]))
    unit = sigma * SCALER   # s in scaled units = s in the caller's units times unit^2
    d = np.r_[np.full(3, SCALER), np.ones(3)]
    for f in range(len(g["rels"]["j"])):
        M = _T12_to_44(g["rels"]["Z"][f][None])[0]
        M[:3, 3] /= SCALER
        info = d[:, None] * sym_lower(g["rels"]["Omega"][f]) * d[None, :] / (unit * unit)
        rb = (int(g["kind"][f]), float(g["scale"][f]) / unit) if g["kind"][f] else None
        s.AddRelativePose(int(hp[g["rels"]["j"][f]]), int(hp[g["rels"]["k"][f]]), M, info, sigma_pixel=sigma,
                          robust=rb)
    return s, poses


@pytest.mark.parametrize("cls", [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor])
def test_facade_is_the_raw_call(built, cls):
    g = cases.scene("r40_gm")
    s, poses = pose_facade(cls, g, 0.7)
    rels = s._relative_arrays()
    assert np.array_equal(rels["robust_kind"], g["kind"]) and (rels["robust_kind"] != 0).any()
    options = Options()
    options.iteration_handle.max_num_iterations = 8
    options.convergence_handle.threshold_step_size = -1.0
    options.convergence_handle.threshold_cost_change = -1.0
    options.trust_region_handle.initial_lambda = 1e-4
    T0 = np.concatenate(s._pose_T_jw, axis=0)
    pf = np.zeros(len(T0), np.uint8)
    pf[list(s._pose_fixed)] = 1
    c_opt = options.to_c()
    c_opt.gauss_newton = 1 if s._use_gauss_newton(options) else 0
    raw = BaPoseGraph(T0, pf, dict(j=rels["j"], k=rels["k"], Z=rels["Z"], Omega=rels["Omega"]))
    raw.set_robust(rels["robust_kind"], rels["robust_scale"])
    rows, conv = raw.solve(c_opt)
    T_raw = raw.poses()
    rs, rw = raw.factor_report()
    raw.close()
    with pytest.raises(RuntimeError, match="SolvePoseGraph has not run"):
        s.GetRelativeWeights()
    summary = Summary()
    assert s.SolvePoseGraph(options, summary) is True
    got = summary.optimization_info_list_
    assert [(r.cost, r.trial_cost, r.damping_term, r.iteration_status) for r in rows] == \
        [(r.cost, r.trial_cost, r.damping_term, int(r.iteration_status)) for r in got]
    assert np.array_equal(np.concatenate(s._pose_T_jw, axis=0), T_raw)
    fs, fw = s.GetRelativeWeights()
    assert np.array_equal(fw, rw) and np.array_equal(fs, rs / (0.7 * SCALER) ** 2)
    _, bad, good = cases.outlier_scene("o40")
    assert fw[bad].max() < 1e-2 and fw[good].min() > 0.8
    # the kernels did something: without them the rows differ
    plain = BaPoseGraph(T0, pf, dict(j=rels["j"], k=rels["k"], Z=rels["Z"], Omega=rels["Omega"]))
    prow, _ = plain.solve(c_opt)
    plain.close()
    assert row_bits(prow) != row_bits(rows)
