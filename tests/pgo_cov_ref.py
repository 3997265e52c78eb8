"""Host reference of the pose graph's covariance blocks and chi-square gate (ba_pgraph_covariance,
ba_pgraph_gate): the definition of include/ba_hip.h in numpy / scipy fp64, no GPU.

H = pgo_robust_ref.system(graph, T) (rel_ref.dense_factors with w Omega), Sigma = H^-1 over the
optimisable poses in the user's order, a fixed pose has zero blocks.  Sigma is computed twice,
numpy.linalg.inv and scipy cho_factor / cho_solve on identity columns; the discrepancy of a
quantity between the two routes is the reference's own noise for it, and the GPU has to lie
within 10 x that noise (floor 1e-12): the factor 10 covers a different, equally valid order of
summation (the protocol of test_gpu_covariance.py).

Errors are relative to the scale of what a quantity is computed FROM:
  a pose block     its largest entry
  Sigma_jk         sqrt(max|Sigma_jj| max|Sigma_kk|); with a fixed member the block is zero by
                   definition, its scale is zero and it has to be zero exactly
  Sigma_E and P    max|Sigma_jj| + max|Ad Sigma_kk Ad^T|  (Sigma_E of neighbours far down a chain
                   is a difference of nearly equal matrices)
  d2               itself
"""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from bundle_adjustment_solver_amd.solver import relative_adjoint, relative_covariance, relative_residual

import pgo_robust_ref
from prior_ref import sym_lower

CHI2_6_999 = 22.46   # chi-square quantile, 6 degrees of freedom, 0.999
FLOOR = 1e-12


def sigma_two_ways(graph, T):
    """-> (Sigma by numpy.linalg.inv, Sigma by Cholesky, the 1-norm condition number of H)"""
    H, _ = pgo_robust_ref.system(graph, T)
    S1 = np.linalg.inv(H)
    S2 = cho_solve(cho_factor(H, lower=True), np.eye(H.shape[0]))
    return S1, S2, float(np.abs(H).sum(axis=0).max() * np.abs(S1).sum(axis=0).max())


def opt_of_pose(graph):
    fixed = np.asarray(graph["pose_fixed"])
    out = np.full(len(fixed), -1, np.int64)
    out[fixed == 0] = np.arange(int((fixed == 0).sum()))
    return out


def block(S, a, b):
    """block (a, b) of Sigma by optimisable index; zero where either pose is fixed"""
    if a < 0 or b < 0:
        return np.zeros((6, 6))
    return S[6 * a:6 * a + 6, 6 * b:6 * b + 6]


def quantities(graph, T, S, pose_sel=(), pairs=(), cands=None):
    """Everything the two calls return, from one Sigma: dict with
    pose (n, 6, 6); cross, rel (p, 6, 6) for `pairs` (a list of (j, k));
    r (c, 6), P (c, 6, 6), d2 (c,), rel_c for cands = dict(j, k, Z, Omega);
    s_pose, s_cross, s_rel, s_relc: the error scale of each block (module docstring)."""
    T = np.asarray(T, np.float64).reshape(-1, 12)
    oi = opt_of_pose(graph)

    def pair(j, k):
        a, b = oi[j], oi[k]
        Sjj, Sjk, Skk = block(S, a, a), block(S, a, b), block(S, b, b)
        Ad = relative_adjoint(T[j], T[k])
        s_rel = np.abs(Sjj).max() + np.abs(Ad @ Skk @ Ad.T).max()
        return Sjk, relative_covariance(T[j], T[k], Sjj, Sjk, Skk), np.sqrt(np.abs(Sjj).max() * np.abs(Skk).max()), s_rel

    out = dict(pose=np.array([block(S, oi[j], oi[j]) for j in pose_sel]).reshape(-1, 6, 6))
    out["s_pose"] = np.abs(out["pose"]).reshape(len(out["pose"]), -1).max(axis=1) if len(out["pose"]) else np.zeros(0)
    pq = [pair(int(j), int(k)) for j, k in pairs]
    out["cross"] = np.array([q[0] for q in pq]).reshape(-1, 6, 6)
    out["rel"] = np.array([q[1] for q in pq]).reshape(-1, 6, 6)
    out["s_cross"] = np.array([q[2] for q in pq])
    out["s_rel"] = np.array([q[3] for q in pq])
    if cands is not None:
        cj, ck = np.asarray(cands["j"]).reshape(-1), np.asarray(cands["k"]).reshape(-1)
        Z = np.asarray(cands["Z"], np.float64).reshape(-1, 12)
        Om = np.asarray(cands["Omega"], np.float64).reshape(-1, 6, 6)
        r, P, d2, s_relc = [], [], [], []
        for c in range(len(cj)):
            _, SE, _, s = pair(int(cj[c]), int(ck[c]))
            r.append(relative_residual(T[cj[c]], T[ck[c]], Z[c]))
            P.append(SE + np.linalg.inv(sym_lower(Om[c])))
            d2.append(r[-1] @ np.linalg.solve(P[-1], r[-1]))
            s_relc.append(s)
        out.update(r=np.array(r).reshape(-1, 6), P=np.array(P).reshape(-1, 6, 6), d2=np.array(d2),
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


def reference(graph, T, pose_sel=(), pairs=(), cands=None):
    """-> (quantities from inv(H), noise per quantity name, cond_1(H)): the noise is the
    discrepancy to the same quantities from the Cholesky route"""
    S1, S2, cond = sigma_two_ways(graph, T)
    q1 = quantities(graph, T, S1, pose_sel, pairs, cands)
    q2 = quantities(graph, T, S2, pose_sel, pairs, cands)
    noise = {key: rel_diff(q2[key], q1[key], None if sk is None else q1[sk]) for key, sk in KEYS if key in q1}
    return q1, noise, cond


def bound(noise):
    return 10.0 * max(noise, FLOOR)


def gate_recipe(name):
    """The gate scene of the issue on pgo_robust_cases' outlier scene `name`: all closures
    removed -> (chain graph, candidates dict(j, k, Z, Omega), is_false (c,) bool)"""
    import pgo_robust_cases as cases
    g, bad, _ = cases.outlier_scene(name)
    cl = cases.closures(g)
    chain = cases.without_factors(g, cl)
    cands = {key: np.asarray(g["rels"][key])[cl] for key in ("j", "k", "Z", "Omega")}
    return chain, cands, np.isin(cl, bad)
