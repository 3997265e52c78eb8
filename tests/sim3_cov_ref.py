"""Host reference of the Sim(3) graph's covariance blocks and 7-DoF chi-square gate
(ba_sim3_covariance, ba_sim3_gate): the definition of include/ba_hip.h in numpy /
scipy fp64, no GPU.  The protocol of pgo_cov_ref.py at width 7.

H = sim3_robust_ref.system(graph, S) (sim3_ref.dense_system with w Omega), Sigma = H^-1 over the
optimisable poses in the user's order, tangent [v; omega; sigma]; a fixed pose has zero blocks.
Sigma is computed twice, numpy.linalg.inv and scipy cho_factor / cho_solve on identity columns;
the discrepancy of a quantity between the two routes is the reference's own noise for it, and the
GPU has to lie within 10 x that noise (floor 1e-12): the factor 10 covers a different, equally
valid order of summation.  Omega_z^-1 of a candidate goes the same two routes (numpy.linalg.inv,
Cholesky), so that the noise of P and d2 holds the conditioning of the 7x7 inverse as well.

Errors are relative to the scale of what a quantity is computed FROM:
  a pose block     its largest entry
  Sigma_jk         sqrt(max|Sigma_jj| max|Sigma_kk|); with a fixed member the block is zero by
                   definition, its scale is zero and it has to be zero exactly
  Sigma_E          max|Sigma_jj| + max|Ad7 Sigma_kk Ad7^T|  (Sigma_E of neighbours far down a chain
                   is a difference of nearly equal matrices)
  P                that plus max|Omega_z^-1|: P is the sum of the two, and either may dwarf the
                   other (a vague candidate on a well-determined pair, a sharp one on a loose pair)
  d2               itself
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

import sim3_ref
import sim3_robust_ref

CHI2_7_999 = 24.32   # chi-square quantile, 7 degrees of freedom, 0.999 (test_sim3_robust_ref.py confirms it)
FLOOR = 1e-12


def sigma_two_ways(graph, S):
    """-> (Sigma by numpy.linalg.inv, Sigma by Cholesky, the 1-norm condition number of H)"""
    H, _ = sim3_robust_ref.system(graph, S)
    S1 = np.linalg.inv(H)
    S2 = cho_solve(cho_factor(H, lower=True), np.eye(H.shape[0]))
    return S1, S2, float(np.abs(H).sum(axis=0).max() * np.abs(S1).sum(axis=0).max())


def opt_of_pose(graph):
    fixed = np.asarray(graph["pose_fixed"])
    out = np.full(len(fixed), -1, np.int64)
    out[fixed == 0] = np.arange(int((fixed == 0).sum()))
    return out


def block(Sg, a, b):
    """block (a, b) of Sigma by optimisable index; zero where either pose is fixed"""
    if a < 0 or b < 0:
        return np.zeros((7, 7))
    return Sg[7 * a:7 * a + 7, 7 * b:7 * b + 7]


def adjoint_of_pair(Sj, Sk):
    return sim3_ref.adjoint(sim3_ref.from_mat(sim3_ref.E_of(Sj, Sk)))


def relative_covariance(Ad, Sjj, Sjk, Skk):
    return Sjj - Sjk @ Ad.T - Ad @ Sjk.T + Ad @ Skk @ Ad.T


def quantities(graph, S, Sg, pose_sel=(), pairs=(), cands=None, cholesky=False):
    """Everything the two calls return, from one Sigma (cholesky: Omega_z^-1 by that route too): dict with
    pose (n, 7, 7); cross, rel (p, 7, 7) for `pairs` (a list of (j, k));
    r (c, 7), P (c, 7, 7), d2 (c,) for cands = dict(j, k, Z, Omega);
    s_pose, s_cross, s_rel, s_relc: the error scale of each block (module docstring)."""
    S = np.asarray(S, np.float64).reshape(-1, 13)
    oi = opt_of_pose(graph)

    def pair(j, k):
        a, b = oi[j], oi[k]
        Sjj, Sjk, Skk = block(Sg, a, a), block(Sg, a, b), block(Sg, b, b)
        Ad = adjoint_of_pair(S[j], S[k])
        s_rel = np.abs(Sjj).max() + np.abs(Ad @ Skk @ Ad.T).max()
        return Sjk, relative_covariance(Ad, Sjj, Sjk, Skk), np.sqrt(np.abs(Sjj).max() * np.abs(Skk).max()), s_rel

    out = dict(pose=np.array([block(Sg, oi[j], oi[j]) for j in pose_sel]).reshape(-1, 7, 7))
    out["s_pose"] = np.abs(out["pose"]).reshape(len(out["pose"]), -1).max(axis=1) if len(out["pose"]) else np.zeros(0)
    pq = [pair(int(j), int(k)) for j, k in pairs]
    out["cross"] = np.array([q[0] for q in pq]).reshape(-1, 7, 7)
    out["rel"] = np.array([q[1] for q in pq]).reshape(-1, 7, 7)
    out["s_cross"] = np.array([q[2] for q in pq])
    out["s_rel"] = np.array([q[3] for q in pq])
    if cands is not None:
        cj, ck = np.asarray(cands["j"]).reshape(-1), np.asarray(cands["k"]).reshape(-1)
        Z = np.asarray(cands["Z"], np.float64).reshape(-1, 13)
        Om = np.asarray(cands["Omega"], np.float64).reshape(-1, 7, 7)
        r, P, d2, s_relc = [], [], [], []
        for c in range(len(cj)):
            _, SE, _, s = pair(int(cj[c]), int(ck[c]))
            r.append(sim3_ref.residual(S[cj[c]], S[ck[c]], Z[c]))
            Oz = sim3_ref.sym_lower(Om[c])
            Oi = cho_solve(cho_factor(Oz, lower=True), np.eye(7)) if cholesky else np.linalg.inv(Oz)
            P.append(SE + Oi)
            d2.append(r[-1] @ np.linalg.solve(P[-1], r[-1]))
            s_relc.append(s + np.abs(Oi).max())
        out.update(r=np.array(r).reshape(-1, 7), P=np.array(P).reshape(-1, 7, 7), d2=np.array(d2),
                   s_relc=np.array(s_relc))
    return out


KEYS = (("pose", "s_pose"), ("cross", "s_cross"), ("rel", "s_rel"), ("P", "s_relc"), ("d2", None))


def rel_diff(a, b, scale):
    """largest over the blocks of max|a - b| / scale (scale None: |b| itself, for d2)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.size == 0:
        return 0.0
    d = np.abs(a - b).reshape(len(a), -1).max(axis=1)
    s = np.abs(b).reshape(len(b), -1).max(axis=1) if scale is None else np.asarray(scale, np.float64)
    # a scale of zero (the cross block with a fixed pose) allows no difference at all
    zero = s == 0.0
    return float(np.where(zero, np.where(d == 0.0, 0.0, np.inf), d / np.where(zero, 1.0, s)).max())


def reference(graph, S, pose_sel=(), pairs=(), cands=None):
    """-> (quantities from inv(H), noise per quantity name, cond_1(H)): the noise is the
    discrepancy to the same quantities from the Cholesky route"""
    S1, S2, cond = sigma_two_ways(graph, S)
    q1 = quantities(graph, S, S1, pose_sel, pairs, cands)
    q2 = quantities(graph, S, S2, pose_sel, pairs, cands, cholesky=True)
    noise = {key: rel_diff(q2[key], q1[key], None if sk is None else q1[sk]) for key, sk in KEYS if key in q1}
    return q1, noise, cond


def bound(noise):
    return 10.0 * max(noise, FLOOR)


def gate_recipe():
    """The gate scene on sim3_robust_cases' outlier scene: all closures removed -> (chain graph,
    candidates dict(j, k, Z, Omega), is_false (c,) bool)"""
    import sim3_robust_cases as cases
    g, bad, _ = cases.outlier_scene()
    cl = cases.closures(g)
    chain = cases.without_factors(g, cl)
    cands = {key: np.asarray(g["rels"][key])[cl] for key in ("j", "k", "Z", "Omega")}
    return chain, cands, np.isin(cl, bad)
