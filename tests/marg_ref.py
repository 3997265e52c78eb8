"""Host reference for the marginalisation-prior tests (numpy / scipy fp64, no GPU).

plan: the numpy restatement of ba_batch_marg_plan_problem — the kept poses and the landmark
set L of one problem under a marking.
reference: the prior (H, b) on the kept poses.  Every observation of a landmark outside L
is dropped, the CPU oracle linearises what is left (lambda = 0), the full normal matrix
[[A, W], [W^T, C]] over the optimisable poses and the landmarks of L is assembled
(cov_ref.full_normal_matrix) with g = [a; b], and {marked poses} U L is eliminated two
ways: (i) one numpy.linalg.solve on the joint block, (ii) the landmarks by their 3x3
inverses, then the marked poses by scipy's Cholesky.  The matrix-wide relative difference
of the two routes is the reference's own noise; route (i) is the reference.
"""
import numpy as np
import scipy.linalg

from bundle_adjustment_solver_amd import scenes
from oracle import oracle_py as O

import cov_ref

OBS_KEYS = ("obs_cam", "obs_pose", "obs_pt", "obs_uv")


def plan(pr, marg):
    """(kept poses ascending, L as one bool per point)"""
    marg = np.asarray(marg) != 0
    pf, qf = np.asarray(pr["pose_fixed"]) != 0, np.asarray(pr["pt_fixed"]) != 0
    in_l = np.zeros(len(qf), bool)
    in_l[np.asarray(pr["obs_pt"])[marg[np.asarray(pr["obs_pose"])]]] = True
    return np.flatnonzero(~pf & ~marg), in_l & ~qf


def rel_diff(x, y):
    """max|x - y| / max|y| over the whole array (0 for a pair of zero arrays)"""
    s, d = (np.abs(y).max(), np.abs(x - y).max()) if y.size else (0.0, 0.0)
    return d / s if s > 0 else (0.0 if d == 0 else np.inf)


def reference(pr, marg, huber=1.0):
    """(H (6K, 6K), b (6K,), noise, kept, L) of one problem dict"""
    marg = np.asarray(marg) != 0
    kept, in_l = plan(pr, marg)
    sub = dict(pr)
    keep_obs = in_l[np.asarray(pr["obs_pt"])]
    for k in OBS_KEYS:
        sub[k] = np.ascontiguousarray(np.asarray(pr[k])[keep_obs])
    o = O.Oracle(sub)
    o.linearize(huber)
    o.damp_invert(0.0)
    A, a = o.get_A()
    Cm, b = o.get_C()
    pi, pj, W = o.get_pairs()
    o.close()
    ps = np.flatnonzero(np.asarray(pr["pose_fixed"]) == 0)
    qs = np.flatnonzero(np.asarray(pr["pt_fixed"]) == 0)
    sel = in_l[qs]
    assert sel[pi].all()
    remap = np.cumsum(sel) - 1
    N, ML = len(ps), int(sel.sum())
    Hf = cov_ref.full_normal_matrix(A, Cm[sel], remap[pi], pj, W)
    g = np.concatenate([a.reshape(-1), b[sel].reshape(-1)])
    cols = lambda js: (6 * np.asarray(js, int)[:, None] + np.arange(6)[None, :]).reshape(-1)
    ik = cols(np.flatnonzero(~marg[ps]))
    im = cols(np.flatnonzero(marg[ps]))
    il = 6 * N + np.arange(3 * ML)
    # (i) the joint block at once
    ie = np.concatenate([im, il])
    if len(ie):
        sol = np.linalg.solve(Hf[np.ix_(ie, ie)], np.column_stack([Hf[np.ix_(ie, ik)], g[ie]]))
        H1 = Hf[np.ix_(ik, ik)] - Hf[np.ix_(ik, ie)] @ sol[:, :-1]
        b1 = g[ik] - Hf[np.ix_(ik, ie)] @ sol[:, -1]
    else:
        H1, b1 = Hf[np.ix_(ik, ik)].copy(), g[ik].copy()
    # (ii) the landmarks by their 3x3 inverses, then the marked poses by Cholesky
    ip = np.arange(6 * N)
    S, r = Hf[np.ix_(ip, ip)].copy(), g[ip].copy()
    for i in range(ML):
        c = 6 * N + 3 * i + np.arange(3)
        Ci = np.linalg.inv(Hf[np.ix_(c, c)])
        V = Hf[np.ix_(ip, c)] @ Ci
        S -= V @ Hf[np.ix_(c, ip)]
        r -= V @ g[c]
    H2, b2 = S[np.ix_(ik, ik)], r[ik]
    if len(im):
        cf = scipy.linalg.cho_factor(S[np.ix_(im, im)], lower=True)
        H2 = H2 - S[np.ix_(ik, im)] @ scipy.linalg.cho_solve(cf, S[np.ix_(im, ik)])
        b2 = b2 - S[np.ix_(ik, im)] @ scipy.linalg.cho_solve(cf, r[im])
    noise = max(rel_diff(H2, H1), rel_diff(b2, b1))
    return H1, b1, noise, kept, in_l


# name -> (n_pose, n_pt, stereo, seed, n_fixed, marked poses, far pose)
SCENES = {
    "mono5_m1": (5, 37, False, 11, 2, (2,), 4),
    "stereo4_m1": (4, 29, True, 12, 1, (1,), 3),
    "mono8_m2": (8, 33, False, 16, 2, (2, 3), 7),
    "stereo12_m3": (12, 40, True, 15, 2, (2, 3, 4), 11),
    "stereo18_m1": (18, 45, True, 13, 2, (2,), 17),
    "mono18_m8": (18, 45, False, 17, 2, tuple(range(2, 10)), 17),
    "stereo16_nofixed_m1": (16, 45, True, 19, 0, (0,), 15),
    "mono16_nofixed_m3": (16, 45, False, 23, 0, (0, 1, 2), 15),
}


def build_scene(name):
    """(scaled problem dict, marking, far pose): a window in which the marked poses see
    only the landmarks [0, 2 n_pt // 3) and the far pose only the others"""
    n_pose, n_pt, stereo, seed, n_fixed, marked, far = SCENES[name]
    sc = scenes.ba_batch_scene(1, n_pose, n_pt, stereo, seed, n_fixed=n_fixed)[0]
    cut = 2 * n_pt // 3
    mk = np.zeros(n_pose, np.uint8)
    mk[list(marked)] = 1
    near = sc["obs_pt"] < cut
    drop = ((mk[sc["obs_pose"]] != 0) & ~near) | ((sc["obs_pose"] == far) & near)
    for k in OBS_KEYS:
        sc[k] = sc[k][~drop]
    return scenes.scaled_problem(sc), mk, far


def image_columns(pr, marg):
    """columns of the LDS image a batch of this problem alone gets: the marked optimisable
    poses padded to whole 16-column tiles, then the kept poses; 32, 64, 96 or 112"""
    marg = np.asarray(marg) != 0
    opt = np.asarray(pr["pose_fixed"]) == 0
    m, K = int((opt & marg).sum()), int((opt & ~marg).sum())
    tiles = max(1, -(-(16 * (-(-6 * m // 16)) + 6 * K) // 16))
    return 16 * next(c for c in (2, 4, 6, 7) if tiles <= c)
