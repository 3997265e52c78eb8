"""GPU tests of the Python facades of the robust kernels, covariance blocks and gate of the Sim(3)
graph (AddRelativeSim3(robust=...), SolveSim3Graph, GetRelativeSim3Weights,
ComputeSim3GraphCovariance, GateSim3LoopClosures of both solver classes) on
sim3_cases.loop_scene: each facade call equals the raw BaSim3Graph call to the bit after the unit
conversion, robust=None reproduces the bits of before, mixed sigma_pixel raises, and SolvePoseGraph,
Solve and SolveBatch do not see the Sim(3) factors, robust or not.
"""
import numpy as np
import pytest

from bundle_adjustment_solver_amd import _lib
from bundle_adjustment_solver_amd.solver import (INVERSE_SCALER, ROBUST_CAUCHY, ROBUST_GEMAN_MCCLURE, ROBUST_HUBER, SCALER,
                                                 BaSim3Graph, Camera, FullBundleAdjustmentSolver,
                                                 FullBundleAdjustmentSolverRefactor, Summary)

import sim3_cases as cases
from test_gpu_sim3_graph import facade_options

pytestmark = pytest.mark.gpu
CLASSES = [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor]
SIGMA = 0.7
KERNELS = [None, (ROBUST_HUBER, 2.0), (ROBUST_CAUCHY, 3.0), (ROBUST_GEMAN_MCCLURE, 4.0)]


def build(cls, sc, robust="cycle", sim3=True, se3=True, sigma=SIGMA):
    """the loop scene in a solver: robust "cycle" puts KERNELS in turn on the Sim(3) factors, None
    adds them as before"""
    s = cls()
    s.AddCamera(0, Camera(*sc["camera"]))
    poses, pts = sc["poses"].copy(), sc["points"].copy()
    hp = s.AddPoseArray(poses)
    hq = s.AddPointArray(pts)
    s.MakePoseFixed(int(hp[0]))
    s.AddObservations(0, hp[sc["obs"][0]], hq[sc["obs"][1]], sc["obs"][2])
    if sim3:
        for f, (j, k, M, Om) in enumerate(sc["factors"]):
            if robust is None:
                s.AddRelativeSim3(int(hp[j]), int(hp[k]), M, Om, sigma_pixel=sigma)
            else:
                s.AddRelativeSim3(int(hp[j]), int(hp[k]), M, Om, sigma_pixel=sigma, robust=KERNELS[f % 4])
    if se3:   # rigid odometry of the drifted map, for SolvePoseGraph and Solve
        rng = np.random.default_rng(3)
        for j, k, M, Om in sc["factors"][:len(poses) - 1]:
            R = M.copy()
            R[:3, :3] /= np.cbrt(np.linalg.det(M[:3, :3]))
            R[:3, 3] += 1e-2 * rng.standard_normal(3)
            s.AddRelativePose(int(hp[j]), int(hp[k]), R, Om[:6, :6], sigma_pixel=sigma)
    return s, poses, pts, hp


def raw_inputs(s):
    T0 = np.concatenate(s._pose_T_jw, axis=0)
    pf = np.zeros(len(T0), np.uint8)
    pf[list(s._pose_fixed)] = 1
    return np.c_[T0, np.ones(len(T0))], pf, s._sim3_arrays()


def bits(rows):
    return [(r.cost, r.trial_cost, r.damping_term, int(r.iteration_status)) for r in rows]


@pytest.mark.parametrize("cls", CLASSES)
def test_robust_solve_and_weights_are_the_raw_calls(built, cls):
    sc = cases.loop_scene()
    s, poses, _, _ = build(cls, sc)
    S0, pf, rels = raw_inputs(s)
    F = len(sc["factors"])
    unit = SIGMA * SCALER
    assert rels["robust_kind"].tolist() == [f % 4 for f in range(F)]
    want_scale = [0.0 if KERNELS[f % 4] is None else KERNELS[f % 4][1] * SIGMA * SCALER for f in range(F)]
    assert rels["robust_scale"].tolist() == want_scale   # times sigma_pixel SCALER
    options = facade_options()
    c_opt = options.to_c()
    c_opt.gauss_newton = 1 if s._use_gauss_newton(options) else 0
    raw = BaSim3Graph(S0, pf, dict(j=rels["j"], k=rels["k"], Z=rels["Z"], Omega=rels["Omega"]))
    raw.set_robust(rels["robust_kind"], rels["robust_scale"])
    rows, conv = raw.solve(c_opt)
    S_raw = raw.poses()
    rs, rw = raw.factor_weights()
    raw.close()
    plain = BaSim3Graph(S0, pf, dict(j=rels["j"], k=rels["k"], Z=rels["Z"], Omega=rels["Omega"]))
    rows_plain, _ = plain.solve(c_opt)
    plain.close()
    with pytest.raises(RuntimeError, match="SolveSim3Graph has not run"):
        s.GetRelativeSim3Weights()
    summary = Summary()
    scales = s.SolveSim3Graph(options, summary, point_anchors=list(sc["anchors"]))
    assert bits(rows) == bits(summary.optimization_info_list_) and bits(rows) != bits(rows_plain)
    assert np.array_equal(scales, S_raw[:, 12])
    gs, gw = s.GetRelativeSim3Weights()
    assert np.array_equal(gs, rs / (unit * unit)) and np.array_equal(gw, rw)
    # (the scene's optimum has zero residuals: the kernels bite on the way, as the rows show, and
    # every weight ends at or next to 1)
    assert np.all(gw[np.arange(F) % 4 == 0] == 1.0) and np.all(gw <= 1.0) and np.all(gs >= 0.0)
    assert not np.array_equal(poses, sc["poses"])
    # one iteration in: the weights of the kernels are below 1, and still the raw call's
    t, _, _, _ = build(cls, sc)
    one = facade_options(1)
    raw = BaSim3Graph(S0, pf, rels)   # the factor dict carries the kernels
    c_one = one.to_c()
    c_one.gauss_newton = c_opt.gauss_newton
    raw.solve(c_one)
    rs1, rw1 = raw.factor_weights()
    raw.close()
    t.SolveSim3Graph(one)
    ts, tw = t.GetRelativeSim3Weights()
    assert np.array_equal(ts, rs1 / (unit * unit)) and np.array_equal(tw, rw1) and tw.min() < 1.0


@pytest.mark.parametrize("cls", CLASSES)
def test_robust_none_reproduces_the_bits_of_before(built, cls):
    sc = cases.loop_scene()
    options = facade_options()
    a, poses_a, pts_a, _ = build(cls, sc, robust=None)
    assert sorted(a._sim3_arrays()) == ["Omega", "Z", "j", "k"]
    S0, pf, rels = raw_inputs(a)
    c_opt = options.to_c()
    c_opt.gauss_newton = 1 if a._use_gauss_newton(options) else 0
    raw = BaSim3Graph(S0, pf, rels)
    rows, _ = raw.solve(c_opt)
    S_raw = raw.poses()
    rep = raw.factor_report()
    raw.close()
    sa = Summary()
    scales_a = a.SolveSim3Graph(options, sa, point_anchors=list(sc["anchors"]))
    assert bits(rows) == bits(sa.optimization_info_list_) and np.array_equal(scales_a, S_raw[:, 12])
    gs, gw = a.GetRelativeSim3Weights()   # without a kernel: s of ba_sim3_factor_report, w = 1
    unit = SIGMA * SCALER
    assert np.array_equal(gs, rep / (unit * unit)) and np.all(gw == 1.0)
    # kind 0 given explicitly is no kernel either
    b = cls()
    hp = b.AddPoseArray(sc["poses"].copy())
    b.MakePoseFixed(int(hp[0]))
    for j, k, M, Om in sc["factors"]:
        b.AddRelativeSim3(int(hp[j]), int(hp[k]), M, Om, sigma_pixel=SIGMA, robust=(0, -1.0))
    sb = Summary()
    scales_b = b.SolveSim3Graph(options, sb)
    assert bits(sb.optimization_info_list_) == bits(rows) and np.array_equal(scales_b, scales_a)
    # a kernel that the check refuses is refused when the factor is added
    j, k, M, Om = sc["factors"][0]
    with pytest.raises(_lib.BaError, match="scale must be > 0"):
        b.AddRelativeSim3(int(hp[j]), int(hp[k]), M, Om, robust=(ROBUST_CAUCHY, 0.0))
    with pytest.raises(_lib.BaError, match="kind = 7"):
        b.AddRelativeSim3(int(hp[j]), int(hp[k]), M, Om, robust=(7, 1.0))
    assert len(b._sim3_relatives) == len(sc["factors"])


@pytest.mark.parametrize("cls", CLASSES)
def test_covariance_and_gate_are_the_raw_calls_in_the_callers_units(built, cls):
    sc = cases.loop_scene()
    s, poses, _, hp = build(cls, sc)
    S0, pf, rels = raw_inputs(s)
    n = len(poses)
    sel = [int(v) for v in np.flatnonzero(pf == 0)[::-3]]
    pairs = [(n - 1, 1), (1, n - 1), (0, 7), (12, 0), (5, 6)]
    cand = [dict(pose_j=int(hp[j]), pose_k=int(hp[k]), measurement=M, information=Om, sigma_pixel=SIGMA,
                 robust=(ROBUST_CAUCHY, 1.0))   # ignored: no robust weight applies to a candidate
            for j, k, M, Om in sc["factors"][-3:]]
    M_bad = sc["factors"][-1][2].copy()
    M_bad[:3, :3] *= 1.3   # the closure with a wrong scale
    cand.append(dict(pose_j=int(hp[sc["factors"][-1][0]]), pose_k=int(hp[sc["factors"][-1][1]]), measurement=M_bad,
                     information=sc["factors"][-1][3], sigma_pixel=SIGMA))
    cz = [s._scaled_sim3(c["measurement"], c["information"], SIGMA) for c in cand]
    raw = BaSim3Graph(S0, pf, dict(j=rels["j"], k=rels["k"], Z=rels["Z"], Omega=rels["Omega"]))
    raw.set_robust(rels["robust_kind"], rels["robust_scale"])
    blocks = raw.covariance(sel, pairs)
    d2 = raw.gate([c["pose_j"] for c in cand], [c["pose_k"] for c in cand], np.array([z[0] for z in cz]),
                  np.array([z[1] for z in cz]))[0]
    raw.close()
    unit = SIGMA * SCALER
    D = np.r_[np.full(3, INVERSE_SCALER), np.ones(4)]
    got = s.ComputeSim3GraphCovariance(sel, pairs)
    for B, G in zip(blocks, got):
        assert G.shape == B.shape and np.array_equal(G, (unit * unit) * (D[None, :, None] * B * D[None, None, :]))
    assert not got[1][2].any() and not got[1][3].any() and got[1][0].any()   # the cross block with the fixed pose
    gd2 = s.GateSim3LoopClosures(cand)
    assert np.array_equal(gd2, d2 / (unit * unit))
    print("d2 of the three closures in place %s, of the closure with 1.3 times the scale %.4g"
          % (gd2[:3], gd2[3]))
    assert gd2[3] != gd2[2] and np.isfinite(gd2).all() and (gd2 > 0).all()
    assert s.is_parameter_finalized_ is False   # neither call finalizes or solves
    assert np.array_equal(np.concatenate(s._pose_T_jw, axis=0), S0[:, :12])
    assert s.ComputeSim3GraphCovariance([], [])[0].shape == (0, 7, 7) and s.GateSim3LoopClosures([]).shape == (0,)


@pytest.mark.parametrize("cls", CLASSES)
def test_mixed_sigma_pixel_raises(built, cls):
    sc = cases.loop_scene()
    s, _, _, hp = build(cls, sc)
    j, k, M, Om = sc["factors"][-1]
    c = dict(pose_j=int(hp[j]), pose_k=int(hp[k]), measurement=M, information=Om)
    with pytest.raises(RuntimeError, match="GateSim3LoopClosures: the factors and candidates were given with "
                                           "sigma_pixel = 0.7 and 1; a covariance in the caller's units needs one value"):
        s.GateSim3LoopClosures([c])
    s.AddRelativeSim3(int(hp[j]), int(hp[k]), M, Om, sigma_pixel=0.5)
    with pytest.raises(RuntimeError, match="ComputeSim3GraphCovariance: the factors and candidates were given with "
                                           "sigma_pixel = 0.7 and 0.5"):
        s.ComputeSim3GraphCovariance([int(hp[3])])
    t = cls()
    t.AddPoseArray(sc["poses"].copy())
    with pytest.raises(RuntimeError, match="AddRelativeSim3"):
        t.ComputeSim3GraphCovariance([1])


@pytest.mark.parametrize("cls", CLASSES)
def test_the_other_solves_do_not_see_robust_sim3_factors(built, cls):
    options = facade_options(4)
    # SolveBatch takes windows of at most 16 optimisable poses: the loop of 12 keyframes for it
    scenes = dict(SolvePoseGraph=cases.loop_scene(), Solve=cases.loop_scene(), SolveBatch=cases.loop_scene(n=12))

    def run(what, sim3):
        sc = scenes[what]
        s, poses, pts, _ = build(cls, sc, sim3=sim3, se3=what != "SolveBatch")
        sm = Summary()
        if what == "SolvePoseGraph":
            assert s.SolvePoseGraph(options, sm) is True
        elif what == "Solve":
            s.Solve(options, sm)
        else:
            res = cls.SolveBatch([s], options, [sm], sigma_pixel=SIGMA)
            assert res[0].status == 0
        return bits(sm.optimization_info_list_), poses, pts

    for what in ("SolvePoseGraph", "Solve", "SolveBatch"):
        (ra, pa, xa), (rb, pb, xb) = run(what, True), run(what, False)
        assert len(ra) > 0 and ra == rb and np.array_equal(pa, pb) and np.array_equal(xa, xb), what
        assert not np.array_equal(pa, scenes[what]["poses"]), what
