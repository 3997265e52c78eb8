"""GPU tests of the Sim(3) graph's covariance blocks and 7-DoF chi-square gate (ba_sim3_covariance,
ba_sim3_gate, BaSim3Graph.covariance / gate; k_graph_cov_rhs and k_graph_cov_solve<Sim3Graph, 32|64> of
csrc/ba_graph_kernels.hip).

Reference: sim3_cov_ref (numpy / scipy fp64) on the seeded scenes of sim3_cases.py and
sim3_robust_cases.py, at the start poses and after the scene's own solve, at the poses the object
holds.  test_sim3_robust_ref.py pins the reference without a GPU.

Bounds: per quantity 10 x max(the reference's own noise (inv(H) against Cholesky), 1e-12), relative
to the scale the quantity is computed from (sim3_cov_ref's docstring); r against
sim3_ref.residual 1e-12.

Sizes: 1 optimisable pose (a group of one, pairs with a fixed member); 4, 5, 9, 10 poses (the
pose-per-tile edges) at both tile orders; 59 poses with fill for pairs inside and across tiles in
both orientations, repeats, a pose in 20 pairs, an odd selection; BA_COV_BATCH 16 and 32 for many
batches.
"""
import numpy as np
import pytest

from bundle_adjustment_solver_amd.solver import BaSim3Graph

import sim3_cases
import sim3_cov_ref as cr
import sim3_ref
import sim3_robust_cases as rcases
from test_gpu_sim3_graph import row_bits

pytestmark = pytest.mark.gpu


def make(g, monkeypatch=None, **env):
    """a graph on a handle of its own; env: BA_* knobs, read by ba_create"""
    for key, v in env.items():
        monkeypatch.setenv(key, str(v))
    p = BaSim3Graph(g["pose_S"], g["pose_fixed"], g["rels"])
    for key in env:
        monkeypatch.delenv(key)
    if "kind" in g:
        p.set_robust(g["kind"], g["scale"])
    return p


def candidates(S, pairs, seed=0, info=50.0):
    """one candidate per pair: the current E = S_j S_k^-1 moved by a tangent step of 0.05, Omega = J^T J"""
    rng = np.random.default_rng(seed)
    Z, Om = [], []
    for j, k in pairs:
        E = sim3_ref.from_mat(sim3_ref.E_of(S[j], S[k]))
        Z.append(sim3_ref.compose(sim3_ref.exp(0.05 * rng.standard_normal(7)), E))
        J = rng.standard_normal((9, 7)) * info
        Om.append(J.T @ J)
    return dict(j=np.array([p[0] for p in pairs], np.int32), k=np.array([p[1] for p in pairs], np.int32),
                Z=np.array(Z).reshape(-1, 13), Omega=np.array(Om).reshape(-1, 7, 7))


def compare(p, g, ps, pairs, tag, cands=None):
    """blocks, cross blocks, Sigma_E, r, P and d2 of the object at the poses it holds against the
    reference; -> the GPU results"""
    S = p.poses()
    cands = candidates(S, pairs) if cands is None else cands
    q, noise, _ = cr.reference(g, S, ps, pairs, cands)
    cp, cc, crel = p.covariance(ps, pairs)
    assert p.dropped_pivots == 0
    d2, r, P = p.gate(cands["j"], cands["k"], cands["Z"], cands["Omega"])
    assert p.dropped_pivots == 0
    got = dict(pose=cp, cross=cc, rel=crel, P=P, d2=d2)
    for key, sk in cr.KEYS:
        err = cr.rel_diff(got[key], q[key], None if sk is None else q[sk])
        print("%s %-5s error %.2e  noise %.2e  bound %.2e" % (tag, key, err, noise[key], cr.bound(noise[key])))
        assert err <= cr.bound(noise[key]), (tag, key, err, noise[key])
    for c in range(len(cands["j"])):
        want = sim3_ref.residual(S[cands["j"][c]], S[cands["k"][c]], cands["Z"][c])
        assert np.abs(r[c] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (tag, c)
    # blocks of the inverse of an SPD matrix: Sigma_jj, Sigma_E and P symmetric to the bit, positive diagonal
    for B in (cp, crel, P):
        assert np.array_equal(B, B.transpose(0, 2, 1))
    assert (np.einsum("nii->ni", cp) > 0).all() and (d2 > 0).all()
    return got


def start_and_solved(name, p, g, ps, pairs, tag=""):
    """at the start poses, then after the scene's own solve"""
    compare(p, g, ps, pairs, name + tag + " start ")
    p.solve(sim3_cases.options(name))
    assert not np.array_equal(p.poses(), g["pose_S"])
    return compare(p, g, ps, pairs, name + tag + " solved")


def all_pairs(g):
    n, fx = len(g["pose_fixed"]), np.asarray(g["pose_fixed"])
    return [(j, k) for j in range(n) for k in range(n) if j != k and not (fx[j] and fx[k])]


# ---- 1. against the reference -----------------------------------------------------------------------
def test_one_optimisable_pose(built):
    """g2: a group of one pose; a pair with a fixed member each way round"""
    g = sim3_cases.scene("g2")
    p = make(g)
    got = start_and_solved("g2", p, g, [1], [(1, 0), (0, 1)])
    # k fixed: Sigma_E = Sigma_jj to the bit; the cross block with a fixed pose is zero
    assert np.array_equal(got["rel"][0], got["pose"][0]) and not got["cross"].any()
    p.close()


@pytest.mark.parametrize("nb", [32, 64])
@pytest.mark.parametrize("name", ["n4", "n5", "n9", "n10"])
def test_pose_per_tile_edges(built, monkeypatch, name, nb):
    """N = 4, 5, 9, 10: a full tile of 4 / 9 poses, one pose into the next; every optimisable pose
    and every pair, those with a fixed member as j and as k among them"""
    g = sim3_cases.scene(name)
    p = make(g, monkeypatch, BA_DENSE_NB=nb)
    assert p.info()["nb"] == nb
    ps = np.flatnonzero(g["pose_fixed"] == 0)
    pairs = all_pairs(g)
    if len(pairs) > 60:   # every pair among the optimisable poses, and each of them with two fixed poses
        fx = np.flatnonzero(g["pose_fixed"] != 0)[:2]
        pairs = [(j, k) for j, k in pairs if (j in ps or j in fx) and (k in ps or k in fx)]
    got = start_and_solved(name, p, g, ps, pairs)
    fixed = np.array([bool(g["pose_fixed"][j] or g["pose_fixed"][k]) for j, k in pairs])
    assert fixed.any() and not got["cross"][fixed].any() and got["cross"][~fixed].any(axis=(1, 2)).all()
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
    orientations, the same pair twice and reversed, a pose in 20 pairs, pairs with the fixed pose
    as j and as k, an odd number of distinct selected poses (a half-filled wave), repeats,
    shuffled order"""
    g = sim3_cases.scene("g60")
    p = make(g, monkeypatch, BA_DENSE_NB=nb)
    assert p.info()["nb"] == nb and p.info()["tiles"] > 2
    ps, pairs = g60_selection()
    assert len(set(ps.tolist())) % 2 == 1
    got = start_and_solved("g60", p, g, ps, pairs, " nb%d" % nb)
    assert np.array_equal(got["pose"][-3], got["pose"][-2])                      # the repeated pose
    assert np.array_equal(got["rel"][6], got["rel"][8])                          # the same pair twice
    assert np.array_equal(got["cross"][6], got["cross"][7].T)                    # reversed: the transposed cross block
    assert not got["cross"][9].any() and not got["cross"][10].any()              # a fixed member: exactly zero
    p.close()


def test_robust_weights_enter_the_system(built):
    """the outlier scene with Geman-McClure on the closures, at its solved poses: the blocks are
    those of the inverse of the WEIGHTED system.  (The 60-pose scenes with their large drift are
    unfit for this: a few iterations in, H can be so ill-conditioned that the reference's two
    routes differ by 5e-7 in Sigma.)"""
    g = rcases.outlier_graph(rcases.ref.GM)
    p = make(g)
    p.solve(rcases.outlier_options())
    w = p.factor_weights()[1]
    assert w.min() < 0.5   # a false closure is down-weighted: the plain system would differ
    ps = np.flatnonzero(g["pose_fixed"] == 0)
    pairs = [(39, 38), (1, 39), (20, 0), (5, 30)]
    got = compare(p, g, ps, pairs, "outlier scene, gm, solved")
    plain = dict(g)
    del plain["kind"], plain["scale"]
    q0 = cr.reference(plain, p.poses(), ps)[0]
    diff = cr.rel_diff(got["pose"], q0["pose"], q0["s_pose"])
    print("outlier scene: the weighted blocks differ from the unweighted reference by %.3g" % diff)
    assert diff > 1e-3
    p.close()


def test_wide_and_narrow_candidates(built):
    """a candidate whose Omega_z^-1 dwarfs Sigma_E (P is the measurement's covariance) and one whose
    Omega_z^-1 vanishes beside it (P is Sigma_E)"""
    g = sim3_cases.scene("g60")
    p = make(g)
    p.solve(sim3_cases.options("g60"))
    S = p.poses()
    pairs = [(59, 1), (59, 1), (30, 0), (30, 0)]
    c = candidates(S, pairs, seed=3)
    c["Omega"][0] *= 1e-10
    c["Omega"][1] *= 1e10
    c["Omega"][2] *= 1e-10
    c["Omega"][3] *= 1e10
    got = compare(p, g, [], [], "wide / narrow", cands=c)
    rel = p.covariance([], pairs)[2]
    inv = np.linalg.inv(sim3_ref.sym_lower(c["Omega"][0]))
    assert np.abs(got["P"][0] - inv).max() <= 1e-6 * np.abs(inv).max()        # Sigma_E is nothing beside it
    assert np.abs(got["P"][1] - rel[1]).max() <= 1e-6 * np.abs(rel[1]).max()  # Omega_z^-1 is nothing beside Sigma_E
    assert got["d2"][0] < got["d2"][1] and got["d2"][2] < got["d2"][3]
    p.close()


# ---- 2. bits ----------------------------------------------------------------------------------------
def test_same_bits_in_any_selection_and_batch_split(built, monkeypatch):
    g = sim3_cases.scene("g60")
    ps, pairs = g60_selection()
    p = make(g)
    p.solve(sim3_cases.options("g60", max_iter=3))
    S = p.poses()
    cands = candidates(S, pairs)
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
    assert [x.shape for x in e] == [(0, 7, 7)] * 3 and p.cov_info()["batches"] == 0 and p.dropped_pivots == 0
    assert p.gate([], [], np.zeros((0, 13)), np.zeros((0, 49)))[0].shape == (0,)
    p.close()
    # many batches: one wave, two waves per batch
    for cols in (16, 32):
        q = make(g, monkeypatch, BA_COV_BATCH=cols)
        q.solve(sim3_cases.options("g60", max_iter=3))
        assert np.array_equal(q.poses(), S)
        c = q.covariance(ps, pairs)
        n_groups = (len(set(ps.tolist())) + 1) // 2 + len(pairs)
        assert q.cov_info()["batch_cols"] == cols and q.cov_info()["batches"] == -(-n_groups // (cols // 16))
        gc = gate(q)
        assert q.cov_info()["batches"] == -(-len(pairs) // (cols // 16))
        assert all(np.array_equal(x, y) for x, y in zip(a + ga, c + gc)), cols
        q.close()


# ---- 3. state ---------------------------------------------------------------------------------------
def test_the_calls_leave_the_object_as_they_found_it(built):
    g = rcases.scene("r60_gm")   # rejected steps among its iterations, robust kernels
    opt = rcases.options("r60_gm")
    ps, pairs = g60_selection()
    a = make(g)
    r1, _ = a.solve(opt)
    r2, _ = a.solve(opt)
    Sa = a.poses()
    b = make(g)
    s1, _ = b.solve(opt)
    Sb1 = b.poses()
    info, ms, rep = b.info(), b.last_ms(), b.factor_weights()
    cov = b.covariance(ps, pairs)
    cands = candidates(Sb1, pairs)
    b.gate(cands["j"], cands["k"], cands["Z"], cands["Omega"])
    assert b.info() == info and b.last_ms() == ms and np.array_equal(b.poses(), Sb1)
    rep2 = b.factor_weights()
    assert np.array_equal(rep[0], rep2[0]) and np.array_equal(rep[1], rep2[1])
    s2, _ = b.solve(opt)
    assert row_bits(s1) == row_bits(r1) and row_bits(s2) == row_bits(r2)
    assert np.array_equal(b.poses(), Sa)
    assert np.isfinite(cov[0]).all()
    a.close()
    b.close()


# ---- 4. the gate end to end -------------------------------------------------------------------------
def test_gate_end_to_end(built):
    """the outlier scene: the chain alone solved on the GPU, every closure gated on the same object.
    Measured on the MI355X: see DESIGN.md §6p."""
    chain, cands, false = cr.gate_recipe()
    p = make(chain)
    p.solve(rcases.outlier_options())
    q, noise, _ = cr.reference(chain, p.poses(), cands=cands)
    d2, r, P = p.gate(cands["j"], cands["k"], cands["Z"], cands["Omega"])
    err = cr.rel_diff(d2, q["d2"], None)
    print("gate: d2 true", np.sort(d2[~false]), "false", d2[false], "; error %.2e noise %.2e" % (err, noise["d2"]))
    assert err <= cr.bound(noise["d2"])
    assert np.array_equal(d2 < cr.CHI2_7_999, q["d2"] < cr.CHI2_7_999)
    assert np.array_equal(d2 < cr.CHI2_7_999, ~false)
    p.close()
