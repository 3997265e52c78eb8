"""Host tests of the robust Sim(3) reference (sim3_robust_ref.py), of the covariance reference
(sim3_cov_ref.py) and of the scenes the GPU tests compare on (sim3_robust_cases.py).  No GPU.

(a) rho and w: w = d rho / d s by central differences, continuity at the Huber knee, w(0) = 1.
(b) fitness of every trajectory scene: each gain ratio of the reference at least 0.1 relative
    away from 0.25 and 0.5, each iteration moves the cost by at least 1e-6 relative, no factor
    with a Huber kernel has s within 1e-6 relative of its knee c^2 at any accepted or trial pose,
    the two host solves agree on the final poses to 1e-8; one rounding of the start poses moves no
    s_f by more than 1e-13 relative (the GPU tests hold s to 1e-12); statuses 0, 1 and 2 all occur,
    and each 60-pose scene holds a rejected step with an accepted one after it.
(c) the outlier scene: with OUTLIER_SCALE the reference separates the closures (false weights
    below the true ones') and Cauchy and Geman-McClure end closer to the clean solve than the
    plain solve; the chain-only gate separates them at the 7-DoF 0.999 quantile.
(d) the quantile: scipy.stats.chi2.ppf(0.999, 7) = 24.3219 (CHI2_7_999 = 24.32).
"""
import numpy as np
import pytest
import scipy.stats

import sim3_cases
import sim3_cov_ref as cr
import sim3_ref
import sim3_robust_cases as cases
import sim3_robust_ref as ref


def test_quantile_of_seven_degrees_of_freedom():
    q = scipy.stats.chi2.ppf(0.999, 7)
    print("chi2.ppf(0.999, 7) = %.6f" % q)
    assert abs(q - 24.3219) < 1e-4 and round(q, 2) == cr.CHI2_7_999


@pytest.mark.parametrize("kind", [ref.HUBER, ref.CAUCHY, ref.GM])
def test_weight_is_the_derivative_of_rho(kind):
    c = 3.0
    for s in (1e-3, 0.5, 8.9, 9.1, 40.0, 1e4):
        h = 1e-6 * s
        d = (ref.rho(kind, c, s + h) - ref.rho(kind, c, s - h)) / (2.0 * h)
        assert abs(d - ref.weight(kind, c, s)) <= 1e-7 * max(1.0, abs(d)), (kind, s)
    assert ref.weight(kind, c, 0.0) == 1.0 and ref.rho(kind, c, 0.0) == 0.0
    if kind == ref.HUBER:
        assert abs(ref.rho(kind, c, 9.0 * (1 + 1e-12)) - ref.rho(kind, c, 9.0)) < 1e-9


def test_kind_zero_is_the_plain_reference():
    g = sim3_cases.scene("n5")
    assert ref.cost(g["pose_S"], g) == sim3_ref.chi2(g["pose_S"], g["rels"])
    H, b = ref.system(g, g["pose_S"])
    H0, b0 = sim3_ref.dense_system(g["pose_fixed"], g["pose_S"], g["rels"])
    assert np.array_equal(H, H0) and np.array_equal(b, b0)


@pytest.mark.parametrize("name", cases.TRAJECTORY)
def test_trajectory_scene_is_fit(name):
    g = cases.scene(name)
    trace = []
    rows, conv, S = ref.lm(g, cases.options(name), trace=trace)
    assert len(rows) == cases.SCENES[name][4] and not conv
    # (the traced run and the shared one agree to rounding only: scipy's expm / logm are threaded)
    assert [r.iteration_status for r in rows] == [r.iteration_status for r in cases.reference(name)[0]]
    kind, scale = ref.kernels(g)
    assert (kind != 0).any()
    prev = ref.cost(g["pose_S"], g)
    for it, r in enumerate(rows):
        change = abs(prev - r.trial_cost) / prev
        margin = min(abs(r.rho - 0.25) / 0.25, abs(r.rho - 0.5) / 0.5)
        print("%s it %d status %d rho %.4f margin %.3f relative change %.3e"
              % (name, it, r.iteration_status, r.rho, margin, change))
        assert margin >= 0.1 and change >= 1e-6
        prev = r.cost
    h = kind == ref.HUBER
    if h.any():   # the accepted and the trial poses of every iteration: the start and one per iteration
        assert len(trace) == len(rows) + 1
        knee = min(np.abs(s[h] / scale[h] ** 2 - 1.0).min() for s in trace)
        print("%s closest approach to a Huber knee: %.3e relative" % (name, knee))
        assert knee >= 1e-6
    noise = sim3_ref.pose_distance(cases.reference_cholesky(name)[2], S)
    print("%s noise of the host reference %.3e" % (name, noise))
    assert noise <= 1e-8


@pytest.mark.parametrize("name", cases.TRAJECTORY)
def test_s_at_the_start_is_conditioned_well_enough_for_its_bound(name):
    """The GPU tests hold s and w at the start poses to 1e-12 relative.  t_E = t_j - (s_j / s_k) R_E
    t_k cancels where the start has drifted far from the origin, and no arithmetic can give s
    better than the rounding of the poses themselves allows: every entry of every pose moved by one
    rounding (a relative 2^-53, random sign) must move no s_f by more than 1e-13 relative."""
    g = cases.scene(name)
    rng = np.random.default_rng(1)
    S = np.asarray(g["pose_S"], np.float64)
    moved = S * (1.0 + 2.0 ** -53 * rng.choice([-1.0, 1.0], S.shape))
    s0, s1 = ref.factor_s(S, g["rels"]), ref.factor_s(moved, g["rels"])
    worst = (np.abs(s1 - s0) / s0).max()
    print("%s: one rounding of the poses moves s by %.2e relative, max |t| %.1f" % (name, worst, np.abs(S[:, 9:12]).max()))
    assert worst <= 1e-13


def test_every_status_occurs():
    seen = set()
    for name in cases.TRAJECTORY:
        seen |= {r.iteration_status for r in cases.reference(name)[0]}
    assert seen == {0, 1, 2}
    for name in cases.SIXTY:   # a rejection, then an accepted step: the records and weights that stayed are used
        st = [r.iteration_status for r in cases.reference(name)[0]]
        assert 2 in st and any(s != 2 for s in st[st.index(2):]), (name, st)


def test_sizes_and_placements():
    counts = {n: len(cases.scene(n)["rels"]["j"]) for n in ("huber_g30_32", "mixed_g30_31", "mixed_g30_33", "one_31")}
    assert counts == dict(huber_g30_32=sim3_cases.FPB, mixed_g30_31=sim3_cases.FPB - 1,
                          mixed_g30_33=sim3_cases.FPB + 1, one_31=sim3_cases.FPB + 1)
    assert np.flatnonzero(cases.scene("one_31")["kind"]).tolist() == [sim3_cases.FPB - 1]
    assert np.flatnonzero(cases.scene("one_32")["kind"]).tolist() == [sim3_cases.FPB]
    assert set(cases.scene("mixed_g30_31")["kind"][:8].tolist()) == {0, 1, 2, 3}
    g = cases.scene("fixed_twin")
    j, k, fx, kd = g["rels"]["j"], g["rels"]["k"], g["pose_fixed"], g["kind"]
    on = np.flatnonzero(kd)
    assert any(fx[j[f]] for f in on) and any(fx[k[f]] for f in on)          # the fixed pose as j and as k
    pairs = [(int(j[f]), int(k[f])) for f in on]
    assert any((b, a) in pairs for a, b in pairs) and 0 < len(on) < len(kd)  # the twin closure, both ways round
    sizes = {n: int((cases.scene(n)["pose_fixed"] == 0).sum()) for n in ("r2", "rn4", "rn5", "rn9", "rn10")}
    assert sizes == dict(r2=1, rn4=4, rn5=5, rn9=9, rn10=10)
    for name in cases.SIXTY:
        assert len(cases.scene(name)["pose_fixed"]) == 60


def test_exact_graph_sits_at_the_truth():
    for kind in (ref.HUBER, ref.CAUCHY, ref.GM):
        g = cases.exact_graph(kind)
        s, w = ref.report(g["pose_S"], g)
        assert s.max() < 1e-20 and np.all(w == 1.0)


def test_outlier_scene_separates_in_the_reference():
    g, bad, good = cases.outlier_scene()
    assert len(g["pose_fixed"]) == 40 and len(bad) == 2 and len(good) == 6
    clean = cases.outlier_clean()
    dist = {kind: sim3_ref.pose_distance(cases.outlier_reference(kind)[2], clean) for kind in (0, 1, 2, 3)}
    for kind in (1, 2, 3):
        gk = cases.outlier_graph(kind)
        _, w = ref.report(cases.outlier_reference(kind)[2], gk)
        print("kind %d: distance to the clean solve %.3e (plain %.3e); weights true %.3g .. %.3g, false %.3g .. %.3g"
              % (kind, dist[kind], dist[0], w[good].min(), w[good].max(), w[bad].min(), w[bad].max()))
        assert w[bad].max() < w[good].min()
    assert dist[2] < dist[0] and dist[3] < dist[0]


def test_gate_separates_in_the_reference():
    chain, cands, false = cr.gate_recipe()
    S = ref.lm(chain, cases.outlier_options())[2]
    q, noise, cond = cr.reference(chain, S, cands=cands)
    print("gate on the chain: d2 true", np.sort(q["d2"][~false]), "false", q["d2"][false], "noise %.2e cond %.2e"
          % (noise["d2"], cond))
    assert (q["d2"][~false] < cr.CHI2_7_999).all() and (q["d2"][false] > cr.CHI2_7_999).all()


def test_covariance_reference_is_consistent():
    """Sigma_E of the reference against a Monte-Carlo free statement: J Sigma J^T with the stacked
    Jacobian [I, -Ad7] of the definition, and the reduced forms with a fixed member"""
    g = sim3_cases.scene("n5")
    S = g["pose_S"]
    S1, S2, cond = cr.sigma_two_ways(g, S)
    oi = cr.opt_of_pose(g)
    free = np.flatnonzero(oi >= 0)
    j, k = int(free[0]), int(free[3])
    q = cr.quantities(g, S, S1, [j], [(j, k), (k, j), (j, 0), (0, j)])
    Ad = cr.adjoint_of_pair(S[j], S[k])
    a, b = oi[j], oi[k]
    J = np.zeros((7, S1.shape[0]))
    J[:, 7 * a:7 * a + 7] = np.eye(7)
    J[:, 7 * b:7 * b + 7] = -Ad
    assert np.abs(q["rel"][0] - J @ S1 @ J.T).max() <= 1e-12 * np.abs(q["rel"][0]).max()
    assert np.abs(q["cross"][0] - q["cross"][1].T).max() <= 1e-12 * np.abs(q["cross"][0]).max()   # inv(H) is symmetric to rounding
    assert np.array_equal(q["rel"][2], q["pose"][0]) and not q["cross"][2].any() and not q["cross"][3].any()
    Ad0 = cr.adjoint_of_pair(S[0], S[j])
    assert np.abs(q["rel"][3] - Ad0 @ q["pose"][0] @ Ad0.T).max() <= 1e-12 * np.abs(q["rel"][3]).max()
