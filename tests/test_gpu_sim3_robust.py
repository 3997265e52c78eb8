"""GPU tests of the robust kernels of the Sim(3) pose graph (ba_sim3_set_robust,
ba_sim3_factor_weights, BaSim3Graph.set_robust / factor_weights; k_s3_lin_robust and
k_s3_assemble_robust of csrc/ba_sim3.hip).

Reference: sim3_robust_ref (numpy fp64, scipy expm / logm: sim3_ref.lm with sum rho for chi-square
and w Omega for Omega) on the seeded scenes of sim3_robust_cases.py, whose fitness for a
trajectory comparison test_sim3_robust_ref.py pins without a GPU.

Sizes: 1, 4, 5, 9, 10, 29 and 59 optimisable poses at both tile orders; 31 / 32 / 33 factors
around one k_s3_lin workgroup of 32 with the single robust factor on either side of the edge.

Tolerances, those of test_gpu_sim3_graph.py: H and g 1e-9 relative, the cost 1e-12 relative, s
and w against the reference 1e-12 relative; trajectories: status identical, lambda 1e-12, cost
and trial cost 1e-7 relative; final poses max_j |sim3_log(S_gpu S_ref^-1)| <= 10 noise + 1e-13,
noise the distance between the numpy-solve and the Cholesky-solve runs of the reference.
"""
import numpy as np
import pytest

from bundle_adjustment_solver_amd._lib import BaError
from bundle_adjustment_solver_amd.solver import ROBUST_CAUCHY, ROBUST_GEMAN_MCCLURE, ROBUST_HUBER, BaSim3Graph

import sim3_cases
import sim3_ref
import sim3_robust_cases as cases
import sim3_robust_ref as ref
from test_gpu_sim3_graph import assert_poses, assert_same_trajectory, relerr, row_bits

pytestmark = pytest.mark.gpu
KINDS = [ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_GEMAN_MCCLURE]


def make(g, kernels=True):
    p = BaSim3Graph(g["pose_S"], g["pose_fixed"], g["rels"])
    if kernels:
        p.set_robust(g["kind"], g["scale"])
    return p


def check_system(g, tag=""):
    """weighted system, cost, s and w at the start poses against the reference -> w"""
    p = make(g)
    H, gr = p.system()
    rH, rg = ref.system(g, g["pose_S"])
    c, rc = p.cost(), ref.cost(g["pose_S"], g)
    s, w = p.factor_weights()
    rs, rw = ref.report(g["pose_S"], g)
    es, ew = np.abs(s - rs) / rs, np.abs(w - rw) / rw
    print(tag, "H", relerr(H, rH), "g", relerr(gr, rg), "cost", abs(c - rc) / rc, "s", es.max(), "w", ew.max(),
          "weights in [%.3g, %.3g]" % (w.min(), w.max()))
    assert relerr(H, rH) < 1e-9 and relerr(gr, rg) < 1e-9
    assert np.array_equal(H, H.T)
    assert abs(c - rc) <= 1e-12 * rc
    assert es.max() <= 1e-12 and ew.max() <= 1e-12
    assert np.array_equal(s, p.factor_report())      # ba_sim3_factor_report keeps its bits
    assert np.array_equal(p.poses(), g["pose_S"])    # none of the calls moves the poses
    p.close()
    return w


def check_trajectory(name, p):
    ref_rows, ref_conv, ref_S = cases.reference(name)
    rows, conv = p.solve(cases.options(name))
    for k, (a, b) in enumerate(zip(rows, ref_rows)):
        print("%s it %d: status %d/%d lambda %.6g/%.6g trial %.12g/%.12g cost %.12g/%.12g rho %.4g/%.4g"
              % (name, k, a.iteration_status, b.iteration_status, a.damping_term, b.damping_term,
                 a.trial_cost, b.trial_cost, a.cost, b.cost, a.rho, b.rho))
    assert_same_trajectory(rows, ref_rows)
    assert conv == ref_conv
    assert_poses(name, p.poses(), ref_S, cases.reference_cholesky(name)[2], p.info())


def report_bounds(g, S, rs):
    """How far s and w of two fp64 evaluations at the SAME poses may lie apart once the residuals
    are small (after a solve s is no longer 1e4 and more, and 1e-12 of s is below the rounding of
    r).  r = sim3_log(S_j S_k^-1 Z^-1) comes from two products and an inverse of 4x4 matrices with
    entries up to max |t|: each leaves an absolute error of a few eps (1 + max |t|) in E Z^-1, the
    logarithm passes it on, and the library and the reference each do it once, so
    |dr| <= d = 64 eps (1 + 2 max |t|).  Then |ds| <= 2 sqrt(s lmax) d + lmax d^2 with lmax the
    largest eigenvalue of Omega, and |dw| <= 2 |ds| / c^2: |w'| <= 1 / c^2 (Cauchy), 2 / c^2
    (Geman-McClure), 1 / (2 c^2) (Huber beyond the knee).  1e-12 relative is added for the
    arithmetic of s and w itself."""
    d = 64.0 * np.finfo(np.float64).eps * (1.0 + 2.0 * np.abs(np.asarray(S)[:, 9:12]).max())
    Om = np.asarray(g["rels"]["Omega"]).reshape(-1, 7, 7)
    lmax = np.array([np.linalg.eigvalsh(sim3_ref.sym_lower(o)).max() for o in Om])
    ds = 2.0 * np.sqrt(rs * lmax) * d + lmax * d * d + 1e-12 * rs
    return ds, 2.0 * ds / np.asarray(g["scale"], np.float64) ** 2 + 1e-12


# ---- 1. system, cost, s and w ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["huber_g30_32", "cauchy_g30_32", "gm_g30_32"])
def test_each_kind_alone_on_every_factor(built, name):
    g = cases.scene(name)
    w = check_system(g, name)
    assert w.max() < 0.5   # the kernel bites on every factor of the drifted start
    p = make(g)
    check_trajectory(name, p)
    p.close()


@pytest.mark.parametrize("name", ["mixed_g30_31", "mixed_g30_33"])
def test_all_kinds_in_turn_inside_one_workgroup(built, name):
    g = cases.scene(name)
    w = check_system(g, name)
    assert np.all(w[g["kind"] == 0] == 1.0) and w[g["kind"] != 0].max() < 1.0
    p = make(g)
    check_trajectory(name, p)
    p.close()


@pytest.mark.parametrize("name,f", [("one_31", 31), ("one_32", 32)])
def test_single_robust_factor_at_the_workgroup_edge(built, name, f):
    """33 factors: the robust factor is the last of the first k_s3_lin workgroup, then the only
    one of the second"""
    g = cases.scene(name)
    p = make(g)
    assert p.info()["fpb"] == 32 and p.info()["factors"] == 33
    w = check_system(g, name)
    assert w[f] < 0.5 and np.all(np.delete(w, f) == 1.0)
    check_trajectory(name, p)
    p.close()


def test_fixed_ends_and_the_twin_closure(built):
    g = cases.scene("fixed_twin")
    w = check_system(g, "fixed_twin")
    on = g["kind"] != 0
    assert np.all(w[~on] == 1.0) and w[on].min() < 0.5
    p = make(g)
    check_trajectory("fixed_twin", p)
    p.close()


def test_two_pose_graph(built):
    g = cases.scene("r2")
    check_system(g, "r2")
    p = make(g)
    check_trajectory("r2", p)
    p.close()


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("name", ["rn4", "rn5", "rn9", "rn10"])
def test_pose_per_tile_edges(built, monkeypatch, name, nb):
    """N = 4, 5, 9, 10 optimisable poses: a full tile of 4 / 9 poses, one pose into the next"""
    monkeypatch.setenv("BA_DENSE_NB", str(nb))   # read by ba_create
    p = make(cases.scene(name))
    monkeypatch.delenv("BA_DENSE_NB")
    info = p.info()
    ppt = nb // 7
    assert info["N"] == int(name[2:]) and info["nb"] == nb and info["tiles"] == (info["N"] + ppt - 1) // ppt
    check_trajectory(name, p)
    p.close()
    if nb == 32:
        check_system(cases.scene(name), name)


# ---- 2. s = 0 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_exact_measurements_at_the_truth_give_unit_weights(built, kind):
    g = cases.exact_graph(kind)
    p = make(g)
    s, w = p.factor_weights()
    print("kind %d: s at the truth max %.3e" % (kind, s.max()))
    assert s.max() <= 1e-18 and np.all(w == 1.0)   # 1 + 1e-18 is 1 in fp64
    H, gr = p.system()
    q = make(g, kernels=False)
    H0, g0 = q.system()
    assert np.array_equal(H, H0) and np.array_equal(gr, g0)   # w = 1.0 exactly: the plain system to the bit
    p.close()
    q.close()


# ---- 3. 60 poses: rejected steps, then accepted ones ----------------------------------------------
@pytest.mark.parametrize("name", cases.SIXTY)
def test_sixty_pose_trajectory_with_rejected_and_accepted_steps(built, name):
    g = cases.scene(name)
    check_system(g, name)   # H, g, the cost, s and w at the start poses, the bounds of every scene
    p = make(g)
    check_trajectory(name, p)
    st = [r.iteration_status for r in cases.reference(name)[0]]
    assert 2 in st and any(s != 2 for s in st[st.index(2):])
    # s and w after the solve, at the object's own poses, as far as the rounding of r allows
    S = p.poses()
    s, w = p.factor_weights()
    rs, rw = ref.report(S, g)
    ds, dw = report_bounds(g, S, rs)
    print(name, "after the solve: s off by %.3g relative, %.3g of its bound; w by %.3g relative, %.3g of its bound"
          % ((np.abs(s - rs) / rs).max(), (np.abs(s - rs) / ds).max(), (np.abs(w - rw) / rw).max(),
             (np.abs(w - rw) / dw).max()))
    assert (np.abs(s - rs) <= ds).all() and (np.abs(w - rw) <= dw).all()
    assert abs(p.cost() - ref.cost(S, g)) <= 1e-12 * ref.cost(S, g) + ds.sum()
    p.close()


# ---- 4. off is off --------------------------------------------------------------------------------
def test_no_kernel_is_the_plain_solver_to_the_bit(built):
    name = "g60"
    g = sim3_cases.scene(name)
    opt = sim3_cases.options(name)
    F = len(g["rels"]["j"])
    plain = BaSim3Graph(g["pose_S"], g["pose_fixed"], g["rels"])
    r0, _ = plain.solve(opt)
    S0, rep0 = plain.poses(), plain.factor_report()
    assert {r.iteration_status for r in r0} == {0, 1, 2}
    plain.close()
    # all kinds 0, with scales that would be refused on a robust factor
    p = BaSim3Graph(g["pose_S"], g["pose_fixed"], g["rels"])
    p.set_robust(np.zeros(F, np.int32), np.full(F, -1.0))
    r1, _ = p.solve(opt)
    assert row_bits(r1) == row_bits(r0) and np.array_equal(p.poses(), S0) and np.array_equal(p.factor_report(), rep0)
    s, w = p.factor_weights()
    assert np.array_equal(s, rep0) and np.all(w == 1.0)
    # a robust solve in between, then kind = NULL
    p.update_values(g["pose_S"])
    p.set_robust(np.full(F, ROBUST_CAUCHY, np.int32), np.full(F, 30.0))
    r2, _ = p.solve(opt)
    assert row_bits(r2) != row_bits(r0)
    p.update_values(g["pose_S"])
    p.set_robust(None)
    r3, _ = p.solve(opt)
    assert row_bits(r3) == row_bits(r0) and np.array_equal(p.poses(), S0) and np.array_equal(p.factor_report(), rep0)
    assert np.all(p.factor_weights()[1] == 1.0)
    p.close()


def test_shrinking_the_scale_between_solves_equals_a_fresh_object(built):
    g = cases.scene("r60_cauchy")
    opt = cases.options("r60_cauchy", max_iter=4)
    p = make(g)
    p.solve(opt)
    S1 = p.poses()
    p.set_robust(g["kind"], 0.25 * g["scale"])   # graduated non-convexity: the next solve from S1 with a smaller c
    r2, _ = p.solve(opt)
    q = BaSim3Graph(S1, g["pose_fixed"], g["rels"])
    q.set_robust(g["kind"], 0.25 * g["scale"])
    r3, _ = q.solve(opt)
    assert row_bits(r2) == row_bits(r3) and np.array_equal(p.poses(), q.poses())
    a, b = p.factor_weights(), q.factor_weights()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    p.close()
    q.close()


def test_update_values_keeps_the_kernels(built):
    g = cases.scene("r60_gm")
    opt = cases.options("r60_gm", max_iter=5)
    p = make(g)
    r1, _ = p.solve(opt)
    S1 = p.poses()
    p.update_values(g["pose_S"], g["rels"]["Z"], g["rels"]["Omega"])
    r2, _ = p.solve(opt)
    assert row_bits(r1) == row_bits(r2) and np.array_equal(p.poses(), S1)
    plain = make(g, kernels=False)
    r0, _ = plain.solve(opt)
    assert row_bits(r0) != row_bits(r1)
    plain.close()
    # a refused call changes nothing
    bad = g["scale"].copy()
    f = int(np.flatnonzero(g["kind"])[0])
    bad[f] = 0.0
    with pytest.raises(BaError, match=r"scale must be > 0 \(factor %d\)" % f):
        p.set_robust(g["kind"], bad)
    p.update_values(g["pose_S"])
    r3, _ = p.solve(opt)
    assert row_bits(r3) == row_bits(r1)
    p.close()


# ---- 5. outliers, end to end ------------------------------------------------------------------------
def test_false_closures_are_down_weighted(built):
    """40 poses, 8 closures, the last 2 false, the kernel on the closures.  Asserted as an
    ordering only: the false closures' weights lie below the true ones', and Cauchy and
    Geman-McClure end closer to the clean solve than the plain solve.  Measured on the MI355X:
    see DESIGN.md §6p."""
    g, bad, good = cases.outlier_scene()
    clean = cases.outlier_clean()
    opt = cases.outlier_options()
    p = make(g, kernels=False)
    p.solve(opt)
    dist = {0: sim3_ref.pose_distance(p.poses(), clean)}
    assert np.all(p.factor_weights()[1] == 1.0)
    for kind in KINDS:   # the same object, back at the start
        gk = cases.outlier_graph(kind)
        p.update_values(g["pose_S"])
        p.set_robust(gk["kind"], gk["scale"])
        p.solve(opt)
        S = p.poses()
        dist[kind] = sim3_ref.pose_distance(S, clean)
        s, w = p.factor_weights()
        print("kind %d: distance to the clean solve %.4g (plain %.4g); weights of the true closures %.3g .. %.3g, of "
              "the false ones %.3g .. %.3g" % (kind, dist[kind], dist[0], w[good].min(), w[good].max(), w[bad].min(),
                                               w[bad].max()))
        assert w[bad].max() < w[good].min()
        ref_S = cases.outlier_reference(kind)[2]
        assert_poses("outlier scene, kind %d" % kind, S, ref_S, cases.outlier_reference(kind, True)[2], p.info())
    assert dist[ROBUST_CAUCHY] < dist[0] and dist[ROBUST_GEMAN_MCCLURE] < dist[0]
    p.close()
