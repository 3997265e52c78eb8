"""GPU tests of the pose graph's covariance blocks and chi-square gate (ba_pgraph_covariance,
ba_pgraph_gate, BaPoseGraph.covariance / gate, ComputePoseGraphCovariance / GateLoopClosures;
k_graph_cov_rhs and k_graph_cov_solve<Se3Graph, 32|64> of csrc/ba_graph_kernels.hip).

Reference: pgo_cov_ref (numpy / scipy fp64) on the seeded scenes of pgo_cases.py, at the start
poses and after the scene's own solve, at the poses the object holds.  test_pgo_cov_ref.py pins
the reference and the fitness of every scene without a GPU.

Bounds: per quantity 10 x the reference's own noise (inv(H) against Cholesky), floor 1e-12,
relative to the scale the quantity is computed from (pgo_cov_ref's docstring); r against
solver.relative_residual 1e-12.

Sizes: 1 optimisable pose (a group of one, pairs with a fixed member); 5, 6, 10, 11 poses (the
pose-per-tile edges) at both tile orders; 59 poses with fill for pairs inside and across tiles in
both orientations, repeats, a pose in 20 pairs, an odd selection; 329 poses in the planner's
order for several levels; BA_COV_BATCH 16 and 32 for many batches.
"""
import numpy as np
import pytest

from bundle_adjustment_solver_amd.solver import (SCALER, BaPoseGraph, FullBundleAdjustmentSolver,
                                                 FullBundleAdjustmentSolverRefactor, covariance_to_user_units,
                                                 relative_residual)

import pgo_cases
import pgo_cov_ref as cr
import pgo_robust_cases as rcases
import rel_ref
from prior_ref import compose, se3_exp
from test_gpu_pose_graph import row_bits

pytestmark = pytest.mark.gpu


def make(g, monkeypatch=None, **env):
    """a graph on a handle of its own; env: BA_* knobs, read by ba_create"""
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))
    p = BaPoseGraph(g["pose_T"], g["pose_fixed"], g["rels"])
    for key in env:
        monkeypatch.delenv(key)
    if "kind" in g:
        p.set_robust(g["kind"], g["scale"])
    return p


def candidates(T, pairs, seed=0):
    """one candidate per pair: the current relative pose moved by a tangent step of 0.05, Omega = J^T J"""
    rng = np.random.default_rng(seed)
    Z, Om = [], []
    for j, k in pairs:
        E = compose(T[j], rel_ref.inverse12(T[k]))
        Z.append(compose(se3_exp(0.05 * rng.standard_normal(6)), E))
        J = rng.standard_normal((8, 6)) * 50.0
        Om.append(J.T @ J)
    return dict(j=np.array([p[0] for p in pairs], np.int32), k=np.array([p[1] for p in pairs], np.int32),
                Z=np.array(Z).reshape(-1, 12), Omega=np.array(Om).reshape(-1, 6, 6))


def compare(p, g, ps, pairs, tag):
    """blocks, cross blocks, Sigma_E, r, P and d2 of the object at the poses it holds against the
    reference; -> the GPU results"""
    T = p.poses()
    cands = candidates(T, pairs)
    q, noise, _ = cr.reference(g, T, ps, pairs, cands)
    cp, cc, crel = p.covariance(ps, pairs)
    assert p.dropped_pivots == 0
    d2, r, P = p.gate(cands["j"], cands["k"], cands["Z"], cands["Omega"])
    assert p.dropped_pivots == 0
    got = dict(pose=cp, cross=cc, rel=crel, P=P, d2=d2)
    for key, sk in cr.KEYS:
        err = cr.rel_diff(got[key], q[key], None if sk is None else q[sk])
        print("%s %-5s error %.2e  noise %.2e  bound %.2e" % (tag, key, err, noise[key], cr.bound(noise[key])))
        assert err <= cr.bound(noise[key]), (tag, key, err, noise[key])
    for c in range(len(pairs)):
        want = relative_residual(T[cands["j"][c]], T[cands["k"][c]], cands["Z"][c])
        assert np.abs(r[c] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (tag, c)
    # blocks of the inverse of an SPD matrix: symmetric to the bit, positive diagonal
    for B in (cp, crel, P):
        assert np.array_equal(B, B.transpose(0, 2, 1))
    assert (np.einsum("nii->ni", cp) > 0).all() and (d2 > 0).all()
    return got


def start_and_solved(name, p, g, ps, pairs, tag=""):
    """at the start poses, then after the scene's own solve"""
    compare(p, g, ps, pairs, name + tag + " start ")
    p.solve(pgo_cases.options(name))
    assert not np.array_equal(p.poses(), g["pose_T"])
    return compare(p, g, ps, pairs, name + tag + " solved")


def all_pairs(g):
    n, fx = len(g["pose_fixed"]), np.asarray(g["pose_fixed"])
    return [(j, k) for j in range(n) for k in range(n) if j != k and not (fx[j] and fx[k])]


# ---- 1. against the reference ---------------------------------------------------------------------
def test_one_optimisable_pose(built):
    """g2: a group of one pose; a pair with a fixed member each way round"""
    g = pgo_cases.scene("g2")
    p = make(g)
    got = start_and_solved("g2", p, g, [1], [(1, 0), (0, 1)])
    # k fixed: Sigma_E = Sigma_jj to the bit; the cross block with a fixed pose is zero
    assert np.array_equal(got["rel"][0], got["pose"][0]) and not got["cross"].any()
    p.close()


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("name", ["n5", "n6", "n10", "g12"])
def test_pose_per_tile_edges(built, monkeypatch, name, nb):
    """N = 5, 6, 10, 11: a full tile of 5 / 10 poses, one pose into the next; every optimisable
    pose and every pair"""
    g = pgo_cases.scene(name)
    p = make(g, monkeypatch, BA_DENSE_NB=nb)
    assert p.info()["nb"] == nb
    ps = np.flatnonzero(g["pose_fixed"] == 0)
    start_and_solved(name, p, g, ps, all_pairs(g))
    p.close()


def g60_selection():
    rng = np.random.default_rng(60)
    hub = [(17, int(k)) for k in rng.permutation(np.r_[1:17, 18:60])[:20]]          # one pose in 20 pairs
    pairs = [(1, 2), (2, 1), (3, 4), (1, 59), (59, 1), (30, 31), (12, 47), (47, 12), (12, 47), (0, 5), (58, 0)] + hub
    ps = np.r_[rng.permutation(np.arange(1, 60))[:33], [7, 7, 59]]                   # shuffled, repeats
    return ps, pairs


@pytest.mark.parametrize("nb", [32, 64])
def test_g60_with_fill(built, monkeypatch, nb):
    """59 poses, closures that fill the factor: pairs inside one tile and across tiles in both
    orientations (pose_col[j] above and below pose_col[k]), the same pair twice and reversed, a
    pose in 20 pairs, pairs with the fixed pose, an odd number of distinct selected poses,
    repeats, shuffled order"""
    g = pgo_cases.scene("g60")
    p = make(g, monkeypatch, BA_DENSE_NB=nb)
    assert p.info()["nb"] == nb and p.info()["tiles"] > 2
    ps, pairs = g60_selection()
    assert len(set(ps.tolist())) % 2 == 1
    got = start_and_solved("g60", p, g, ps, pairs, " nb%d" % nb)
    assert np.array_equal(got["pose"][-3], got["pose"][-2])                      # the repeated pose
    assert np.array_equal(got["rel"][6], got["rel"][8])                          # the same pair twice
    assert np.array_equal(got["cross"][6], got["cross"][7].T)                    # reversed: the transposed cross block
    p.close()


def test_g330_in_the_planners_order(built):
    g = pgo_cases.scene("g330")
    p = make(g)
    assert p.info()["levels"] > 2
    rng = np.random.default_rng(330)
    pairs = [(329, 328), (328, 327), (1, 329)] + [tuple(int(v) for v in rng.choice(np.arange(1, 330), 2, replace=False))
                                                  for _ in range(17)]
    ps = rng.permutation(np.arange(1, 330))[:41]
    start_and_solved("g330", p, g, ps, pairs)
    p.close()


def test_robust_weights_enter_the_system(built):
    """r40_gm at its solved poses: the blocks are those of the inverse of the WEIGHTED system"""
    g = rcases.scene("r40_gm")
    p = make(g)
    p.solve(rcases.options("r40_gm"))
    w = p.factor_report()[1]
    assert w.min() < 0.5   # a false closure is down-weighted: the plain system would differ
    ps = np.flatnonzero(g["pose_fixed"] == 0)
    pairs = [(39, 38), (1, 39), (20, 0), (5, 30)]
    got = compare(p, g, ps, pairs, "r40_gm solved")
    plain = dict(g)
    del plain["kind"], plain["scale"]
    q0 = cr.reference(plain, p.poses(), ps)[0]
    assert cr.rel_diff(got["pose"], q0["pose"], q0["s_pose"]) > 1e-3
    p.close()


# ---- 2. bits --------------------------------------------------------------------------------------
def test_same_bits_in_any_selection_and_batch_split(built, monkeypatch):
    g = pgo_cases.scene("g60")
    ps, pairs = g60_selection()
    p = make(g)
    p.solve(pgo_cases.options("g60", max_iter=3))
    T = p.poses()
    cands = candidates(T, pairs)
    gate = lambda o, c=cands: o.gate(c["j"], c["k"], c["Z"], c["Omega"])   # noqa: E731
    a, b = p.covariance(ps, pairs), p.covariance(ps, pairs)
    ga, gb = gate(p), gate(p)
    assert all(np.array_equal(x, y) for x, y in zip(a + ga, b + gb))          # run to run
    info = p.cov_info()
    assert info["batches"] == 1 and info["cols_per_wave"] == 16
    # alone: one pose, one pair, one candidate
    one = p.covariance([int(ps[5])], [pairs[12]])
    assert np.array_equal(one[0][0], a[0][5]) and np.array_equal(one[1][0], a[1][12]) and \
        np.array_equal(one[2][0], a[2][12])
    c1 = {key: v[12:13] for key, v in cands.items()}
    g1 = gate(p, c1)
    assert all(np.array_equal(x[0], y[12]) for x, y in zip(g1, ga))
    # the empty selection: returns, writes nothing, runs no batch
    e = p.covariance([], None)
    assert [x.shape for x in e] == [(0, 6, 6)] * 3 and p.cov_info()["batches"] == 0 and p.dropped_pivots == 0
    assert p.gate([], [], np.zeros((0, 12)), np.zeros((0, 36)))[0].shape == (0,)
    p.close()
    # many batches: one wave, two waves per batch
    for cols in (16, 32):
        q = make(g, monkeypatch, BA_COV_BATCH=cols)
        q.solve(pgo_cases.options("g60", max_iter=3))
        assert np.array_equal(q.poses(), T)
        c = q.covariance(ps, pairs)
        n_groups = (len(set(ps.tolist())) + 1) // 2 + len(pairs)
        assert q.cov_info()["batch_cols"] == cols and q.cov_info()["batches"] == -(-n_groups // (cols // 16))
        gc = gate(q)
        assert q.cov_info()["batches"] == -(-len(pairs) // (cols // 16))
        assert all(np.array_equal(x, y) for x, y in zip(a + ga, c + gc)), cols
        q.close()


# ---- 3. state -------------------------------------------------------------------------------------
def test_the_calls_leave_the_object_as_they_found_it(built):
    g = rcases.scene("r60_gm")   # rejected steps among its iterations, robust kernels
    opt = rcases.options("r60_gm")
    ps, pairs = g60_selection()
    a = make(g)
    r1, _ = a.solve(opt)
    r2, _ = a.solve(opt)
    Ta = a.poses()
    b = make(g)
    s1, _ = b.solve(opt)
    Tb1 = b.poses()
    info, ms, rep = b.info(), b.last_ms(), b.factor_report()
    cov = b.covariance(ps, pairs)
    cands = candidates(Tb1, pairs)
    b.gate(cands["j"], cands["k"], cands["Z"], cands["Omega"])
    assert b.info() == info and b.last_ms() == ms and np.array_equal(b.poses(), Tb1)
    rep2 = b.factor_report()
    assert np.array_equal(rep[0], rep2[0]) and np.array_equal(rep[1], rep2[1])
    s2, _ = b.solve(opt)
    assert row_bits(s1) == row_bits(r1) and row_bits(s2) == row_bits(r2)
    assert np.array_equal(b.poses(), Ta)
    assert np.isfinite(cov[0]).all()
    a.close()
    b.close()


# ---- 4. the gate end to end -----------------------------------------------------------------------
def test_gate_end_to_end(built):
    """o40: the chain alone solved on the GPU, every closure gated on the same object"""
    chain, cands, false = cr.gate_recipe("o40")
    p = make(chain)
    p.solve(rcases.outlier_options())
    q, noise, _ = cr.reference(chain, p.poses(), cands=cands)
    d2, r, P = p.gate(cands["j"], cands["k"], cands["Z"], cands["Omega"])
    err = cr.rel_diff(d2, q["d2"], None)
    print("o40 gate: d2 true <= %.2f false >= %.3g; error %.2e noise %.2e" % (d2[~false].max(), d2[false].min(), err,
                                                                            noise["d2"]))
    assert err <= cr.bound(noise["d2"])
    assert np.array_equal(d2 < cr.CHI2_6_999, q["d2"] < cr.CHI2_6_999)
    assert np.array_equal(d2 < cr.CHI2_6_999, ~false)
    p.close()


# ---- 5. facades -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor])
def test_facade_is_the_raw_call_in_the_callers_units(built, cls):
    from bundle_adjustment_solver_amd import scenes
    from test_gpu_relative import facade
    sc = scenes.synthetic_ba_scene(12, 150, 5, True, seed=12)
    nf = int(np.asarray(sc["pose_fixed"]).sum())
    edges = [(q + 1, q) for q in range(nf - 1, 11)] + [(11, nf + 1), (nf, 9)]
    sigma = 0.7
    s, facs, poses, _ = facade(cls, sc, edges, sigma)
    T0 = np.concatenate(s._pose_T_jw, axis=0)
    pf = np.zeros(len(T0), np.uint8)
    pf[list(s._pose_fixed)] = 1
    sel = [int(v) for v in np.flatnonzero(pf == 0)[::-1]]
    pairs = [(11, nf), (nf, 11), (nf - 1, 7)]
    cand = [dict(f, sigma_pixel=sigma) for f in facs[-2:]] + \
        [dict(pose_j=7, pose_k=nf - 1, measurement=np.linalg.inv(poses[7]) @ poses[nf - 1], information=40.0 * np.eye(6),
              sigma_pixel=sigma)]
    sr = cls._scaled_relatives("test", [s], [cand], sigma)[0]
    raw = BaPoseGraph(T0, pf, s._relative_arrays())
    blocks = raw.covariance(sel, pairs)
    d2 = raw.gate(sr["j"], sr["k"], sr["Z"], sr["Omega"])[0]
    raw.close()
    unit = sigma * SCALER
    D = np.r_[np.full(3, 100.0), np.ones(3)]
    got = s.ComputePoseGraphCovariance(sel, pairs)
    for B, G in zip(blocks, got):
        want = unit * unit * D[None, :, None] * B * D[None, None, :]
        assert np.abs(G - want).max() <= 1e-12 * np.abs(want).max()
        assert np.array_equal(G, covariance_to_user_units(B, np.zeros((0, 3, 3)), sigma)[0])
    gd2 = s.GateLoopClosures(cand)
    assert np.abs(gd2 - d2 / (unit * unit)).max() <= 1e-12 * np.abs(gd2).max()
    assert s.is_parameter_finalized_ is False   # neither call finalizes or solves
    assert np.array_equal(np.concatenate(s._pose_T_jw, axis=0), T0)
