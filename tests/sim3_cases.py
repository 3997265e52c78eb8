"""Seeded Sim(3) pose graphs for the Sim(3) tests (scaled units, no GPU): the generator of
pgo_cases.py at width 7.

Truth is pgo_cases.walk, rigid, every scale 1.  Z is the true E = S_j S_k^-1 moved by a small
tangent step in all seven components, Omega = J^T J from a random 9 x 7 J with column weights
1, 1, 1, 3, 3, 3, 2.  The start is the odometry integrated with drift in all seven components
from pose 0, so it drifts in scale too; every fixed pose sits at its truth.  The factors are the
chain (q + 1, q) and then the closures of pgo_cases.closure_pairs: alternating orientation, one
from the fixed pose 0, and the first closure's pair named a second time the other way round.

SCENES: name -> (graph arguments, option arguments, iterations).  The iteration counts are capped
so that every gain ratio of the reference stays clear of 0.25 and 0.5 and every iteration still
moves chi-square (test_sim3_ref.py pins both).
"""
import functools

import numpy as np

from bundle_adjustment_solver_amd._lib import make_options

import pgo_cases
import sim3_ref

FPB = 32   # factors per k_s3_lin workgroup (ba_sim3_info reports it; the GPU tests compare)
WEIGHTS = np.array([1.0, 1.0, 1.0, 3.0, 3.0, 3.0, 2.0])


def graph(n, n_closure=0, seed=0, n_fixed=1, drift=0.03, tangent=1e-2, exact=False, start_off=None,
          twice=True, min_gap=None, info=100.0):
    rng = np.random.default_rng(seed)
    truth = np.c_[pgo_cases.walk(n, rng), np.ones(n)]
    fixed = np.zeros(n, np.uint8)
    fixed[:n_fixed] = 1
    min_gap = max(2, min(n // 3, 100)) if min_gap is None else min_gap
    pairs = [(q + 1, q) for q in range(n - 1)]
    cl = pgo_cases.closure_pairs(n, n_closure, rng, min_gap) if n_closure else []
    pairs += cl
    if cl and twice:
        pairs.append((cl[0][1], cl[0][0]))
    pairs = [(j, k) for j, k in pairs if not (fixed[j] and fixed[k])]
    Z, Om = [], []
    for j, k in pairs:
        E = sim3_ref.from_mat(sim3_ref.E_of(truth[j], truth[k]))
        Z.append(E if exact else sim3_ref.compose(sim3_ref.exp(tangent * rng.standard_normal(7) / np.sqrt(7)), E))
        J = rng.standard_normal((9, 7)) * info * WEIGHTS[None, :]
        Om.append(J.T @ J)
    rels = dict(j=np.array([p[0] for p in pairs], np.int32), k=np.array([p[1] for p in pairs], np.int32),
                Z=np.array(Z).reshape(-1, 13), Omega=np.array(Om).reshape(-1, 7, 7))
    start = truth.copy()
    if start_off is not None:
        for q in range(n):
            if not fixed[q]:
                start[q] = sim3_ref.compose(sim3_ref.exp(start_off * rng.standard_normal(7) / np.sqrt(7)), truth[q])
    else:
        odo = {}
        for f, (j, k) in enumerate(pairs):
            if j == k + 1 and (j, k) not in odo:
                odo[(j, k)] = rels["Z"][f]
        for q in range(1, n):
            if fixed[q]:
                continue
            Zq = odo.get((q, q - 1), sim3_ref.from_mat(sim3_ref.E_of(truth[q], truth[q - 1])))
            start[q] = sim3_ref.compose(sim3_ref.exp(drift * rng.standard_normal(7) / np.sqrt(7)),
                                        sim3_ref.compose(Zq, start[q - 1]))
    return dict(pose_S=start, pose_fixed=fixed, rels=rels, truth=truth)


LM = dict(thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4)
SCENES = {
    "g2": (dict(n=2, seed=1, drift=0.1), LM, 2),
    # 4, 5, 9 and 10 optimisable poses: a full tile of 4 / 9 poses, one pose into the next
    "n4": (dict(n=12, n_closure=3, seed=2, n_fixed=8, min_gap=2, drift=0.5), LM, 3),
    "n5": (dict(n=12, n_closure=3, seed=3, n_fixed=7, min_gap=2, drift=0.5), LM, 3),
    "n9": (dict(n=12, n_closure=3, seed=4, n_fixed=3, min_gap=3, drift=0.5), LM, 3),
    "n10": (dict(n=12, n_closure=3, seed=5, n_fixed=2, min_gap=3, drift=0.5), LM, 3),
    # 31, 32 and 33 factors around one k_s3_lin workgroup: 29 chain factors + 1, 2, 3 closures + the twin
    "g30_31": (dict(n=30, n_closure=1, seed=21, drift=0.5), LM, 4),
    "g30_32": (dict(n=30, n_closure=2, seed=22, drift=0.5), LM, 4),
    "g30_33": (dict(n=30, n_closure=3, seed=23, drift=0.5), LM, 4),
    "g60_63": (dict(n=60, n_closure=3, seed=6, drift=1.5), LM, 8),
    "g60": (dict(n=60, n_closure=4, seed=7, drift=1.5), LM, 10),
    "g60_gn": (dict(n=60, n_closure=4, seed=7), dict(LM, gauss_newton=True), 5),
}
TRAJECTORY = tuple(SCENES)
# noise-free: exact Z, start 1e-3 off the truth
EXACT = {
    "x12": dict(n=12, n_closure=3, seed=11, exact=True, start_off=1e-3, min_gap=3),
    "x60": dict(n=60, n_closure=6, seed=12, exact=True, start_off=1e-3),
}
# positive thresholds: the stop test, on the graph of g60_gn (small drift: LM converges)
STOP = dict(scene="g60_gn", opt=dict(thr_step=1e-5, thr_cost=1e-3, lambda0=1e-4, max_iter=30))


def loop_scene(n=40, per_kf=3, drift=0.003, seed=31):
    """The facade scene in the caller's units: a loop of n rigid keyframes on a circle whose map
    drifted in scale by c_q = exp(drift q) (3 % per 10 keyframes), with per_kf landmarks anchored
    to each keyframe.  The start is the rigid odometry of the drifted map: relative rotations
    true, relative translations c_q times the true ones.  Chain measurements are the exact
    similarities (R_E, c_q t_E, c_q / c_(q-1)), three closures join the ends with
    (R_E, c_j t_E, c_j / c_k): the zero-residual optimum is S_q = (R_q, c_q t_q, c_q), whose
    rigid form [R_q, t_q] is the truth.
    -> dict: poses (n, 4, 4) keyframe poses as AddPose takes them, truth (n, 4, 4), scale (n,),
    factors [(j, k, measurement 4x4, information 7x7)], points (n per_kf, 3), anchors, camera
    (fx, fy, cx, cy), obs (pose, point, pixel)."""
    rng = np.random.default_rng(seed)
    a = 2.0 * np.pi * np.arange(n) / n
    T_wj = np.zeros((n, 4, 4))
    for q in range(n):
        T_wj[q] = np.eye(4)
        T_wj[q, :3, :3] = [[np.cos(a[q]), 0.0, np.sin(a[q])], [0.0, 1.0, 0.0], [-np.sin(a[q]), 0.0, np.cos(a[q])]]
        T_wj[q, :3, 3] = [5.0 * np.cos(a[q]), 0.1 * np.sin(3.0 * a[q]), 5.0 * np.sin(a[q])]
    T_jw = np.linalg.inv(T_wj)
    c = np.exp(drift * np.arange(n))

    def rel(j, k):   # the measured similarity between the drifted keyframes j and k
        E = T_jw[j] @ np.linalg.inv(T_jw[k])
        M = np.eye(4)
        M[:3, :3] = (c[j] / c[k]) * E[:3, :3]
        M[:3, 3] = c[j] * E[:3, 3]
        return E, M

    start = [T_jw[0]]
    for q in range(1, n):
        E = rel(q, q - 1)[0].copy()
        E[:3, 3] *= c[q]
        start.append(E @ start[-1])
    pairs = [(q, q - 1) for q in range(1, n)] + [(n - 1, 0), (n - 2, 1), (2, n - 3)]
    factors = []
    for j, k in pairs:
        J = rng.standard_normal((9, 7)) * WEIGHTS[None, :]
        factors.append((j, k, rel(j, k)[1], J.T @ J))
    poses = np.linalg.inv(np.array(start))
    local = np.c_[rng.uniform(-1.0, 1.0, (n * per_kf, 2)), rng.uniform(2.0, 6.0, n * per_kf)]
    anchors = np.repeat(np.arange(n), per_kf)
    points = np.einsum("nij,nj->ni", poses[anchors, :3, :3], local) + poses[anchors, :3, 3]
    camera = (500.0, 500.0, 320.0, 240.0)
    obs_pose = np.r_[anchors, (anchors + 1) % n]
    obs_pt = np.r_[np.arange(len(points)), np.arange(len(points))]
    return dict(poses=poses, truth=T_wj, scale=c, factors=factors, points=points, anchors=anchors, camera=camera,
                obs=(obs_pose, obs_pt, project(camera, poses[obs_pose], points[obs_pt])))


def project(camera, poses_wj, X):
    """pixels of the points X (n, 3) in the keyframes poses_wj (n, 4, 4; AddPose's convention)"""
    T = np.linalg.inv(poses_wj)
    Xc = np.einsum("nij,nj->ni", T[:, :3, :3], X) + T[:, :3, 3]
    return np.c_[camera[0] * Xc[:, 0] / Xc[:, 2] + camera[2], camera[1] * Xc[:, 1] / Xc[:, 2] + camera[3]]


@functools.lru_cache(maxsize=None)
def scene(name):
    return graph(**(EXACT[name] if name in EXACT else SCENES[name][0]))


def options(name, **over):
    kw = dict(SCENES[name][1], max_iter=SCENES[name][2])
    kw.update(over)
    return make_options(**kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(rows, converged, poses) of sim3_ref.lm on the scene with its options; shared, read-only"""
    return sim3_ref.lm(scene(name), options(name))


@functools.lru_cache(maxsize=None)
def reference_cholesky(name):
    return sim3_ref.lm(scene(name), options(name), sim3_ref.solve_cholesky)


@functools.lru_cache(maxsize=None)
def stop_reference():
    return sim3_ref.lm(scene(STOP["scene"]), make_options(**STOP["opt"]))


@functools.lru_cache(maxsize=None)
def stop_reference_cholesky():
    return sim3_ref.lm(scene(STOP["scene"]), make_options(**STOP["opt"]), sim3_ref.solve_cholesky)
