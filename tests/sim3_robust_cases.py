"""Seeded Sim(3) pose graphs with robust kernels and false closures (scaled units, no GPU), built
on sim3_cases.graph as pgo_robust_cases is on pgo_cases.graph.  A graph here is the dict of
sim3_cases with two more keys, kind (F,) and scale (F,), which sim3_robust_ref reads.

corrupt(g, n_bad): the last n_bad factors (closures: sim3_cases appends them after the chain; the
scenes that use it are built without the twin) become false closures, in order, from one generator:
    rng = np.random.default_rng(5)
    Z <- compose(sim3_ref.exp(np.r_[5 * randn(3), 0.5 * randn(3), 0.3 * randn()]), Z)

OUTLIER: the outlier scene of DESIGN.md §6p: 40 poses, 8 closures of which the last 2 are false,
the kernel on the closures only, scale OUTLIER_SCALE, 12 iterations (test_sim3_robust_ref.py pins
that the scale separates the closures).
SCENES: the trajectory scenes the GPU is compared on: name -> (graph arguments, false closures,
kernel placement, option arguments, iterations).  The iteration counts are capped so that every
gain ratio of the reference stays clear of 0.25 and 0.5, every iteration still moves the cost and
no factor sits on a Huber knee (test_sim3_robust_ref.py pins all three).
"""
import functools

import numpy as np

from bundle_adjustment_solver_amd._lib import make_options

import sim3_cases
import sim3_ref
import sim3_robust_ref as ref

SCALE = 30.0


def corrupt(g, n_bad, seed=5):
    rng = np.random.default_rng(seed)
    Z = np.array(g["rels"]["Z"], np.float64)
    F = Z.shape[0]
    for f in range(F - n_bad, F):
        step = np.r_[5.0 * rng.standard_normal(3), 0.5 * rng.standard_normal(3), 0.3 * rng.standard_normal()]
        Z[f] = sim3_ref.compose(sim3_ref.exp(step), Z[f])
    return dict(g, rels=dict(g["rels"], Z=Z))


def closures(g):
    """the factors that are not chain factors (q + 1, q)"""
    j, k = np.asarray(g["rels"]["j"], np.int64), np.asarray(g["rels"]["k"], np.int64)
    return np.flatnonzero(j != k + 1)


def fixed_and_twin(g):
    """the factors that touch a fixed pose, and every factor whose pair is named a second time"""
    j, k = np.asarray(g["rels"]["j"], np.int64), np.asarray(g["rels"]["k"], np.int64)
    fx = np.asarray(g["pose_fixed"]) != 0
    key = [(min(a, b), max(a, b)) for a, b in zip(j.tolist(), k.tolist())]
    twin = np.array([key.count(q) > 1 for q in key])
    return np.flatnonzero(fx[j] | fx[k] | twin)


def with_kernels(g, kind, where, scale=SCALE):
    """where: "closures", "all", "mixed" (kinds 0, 1, 2, 3 in turn over all factors, `kind`
    unused), "fixed_twin" or an index array"""
    F = len(g["rels"]["j"])
    kd = np.zeros(F, np.int32)
    if isinstance(where, str) and where == "mixed":
        kd[:] = np.arange(F) % 4
    elif isinstance(where, str) and where == "all":
        kd[:] = kind
    elif isinstance(where, str) and where == "closures":
        kd[closures(g)] = kind
    elif isinstance(where, str) and where == "fixed_twin":
        kd[fixed_and_twin(g)] = kind
    else:
        kd[np.asarray(where, np.int64)] = kind
    return dict(g, kind=kd, scale=np.full(F, float(scale)))


def without_factors(g, drop):
    keep = np.setdiff1d(np.arange(len(g["rels"]["j"])), drop)
    return dict(g, rels={key: np.asarray(v)[keep] for key, v in g["rels"].items()})


LM = dict(thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4)
OUTLIER = (dict(n=40, n_closure=8, seed=21, drift=0.03, twice=False), 2)
OUTLIER_SCALE = 30.0
OUTLIER_ITERATIONS = 12


@functools.lru_cache(maxsize=None)
def outlier_scene():
    """-> (corrupted graph without kernels, indices of the false closures, the inlier closures)"""
    args, n_bad = OUTLIER
    g = corrupt(sim3_cases.graph(**args), n_bad)
    F = len(g["rels"]["j"])
    bad = np.arange(F - n_bad, F)
    return g, bad, np.setdiff1d(closures(g), bad)


def outlier_options():
    return make_options(max_iter=OUTLIER_ITERATIONS, **LM)


def outlier_graph(kind):
    g = outlier_scene()[0]
    return with_kernels(g, kind, "closures", OUTLIER_SCALE) if kind else g


@functools.lru_cache(maxsize=None)
def outlier_clean():
    """poses of the plain solve with the false closures removed"""
    g, bad, _ = outlier_scene()
    return ref.lm(without_factors(g, bad), outlier_options())[2]


@functools.lru_cache(maxsize=None)
def outlier_reference(kind, cholesky=False):
    """(rows, converged, poses) of the reference with `kind` on the closures (0: none)"""
    return ref.lm(outlier_graph(kind), outlier_options(), ref.solve_cholesky if cholesky else ref.solve_numpy)


G = sim3_cases.SCENES
# name -> (graph arguments, false closures, (kind, where[, scale]), option arguments, iterations)
SCENES = {
    # each kind alone on every factor of the 32-factor graph (one full k_s3_lin workgroup)
    "huber_g30_32": (G["g30_32"][0], 0, (ref.HUBER, "all"), LM, 4),
    "cauchy_g30_32": (G["g30_32"][0], 0, (ref.CAUCHY, "all"), LM, 4),
    "gm_g30_32": (G["g30_32"][0], 0, (ref.GM, "all"), LM, 4),
    # kinds 0, 1, 2, 3 in turn inside one workgroup, 31 and 33 factors
    "mixed_g30_31": (G["g30_31"][0], 0, (0, "mixed"), LM, 4),
    "mixed_g30_33": (G["g30_33"][0], 0, (0, "mixed"), LM, 4),
    # one robust factor: the last of the first k_s3_lin workgroup, the first of the second
    "one_31": (G["g30_33"][0], 0, (ref.CAUCHY, [31]), LM, 4),
    "one_32": (G["g30_33"][0], 0, (ref.GM, [32]), LM, 4),
    # the factors that touch the fixed pose (as j and as k) and the twin closure
    "fixed_twin": (G["g30_33"][0], 0, (ref.HUBER, "fixed_twin", 100.0), LM, 5),
    "r2": (dict(n=2, seed=1, drift=0.5), 0, (ref.CAUCHY, "all", 1.0), LM, 2),
    # N = 4, 5, 9, 10 optimisable poses (the pose-per-tile edges of both tile orders)
    "rn4": (G["n4"][0], 0, (0, "mixed"), LM, 3),
    "rn5": (G["n5"][0], 0, (0, "mixed"), LM, 3),
    "rn9": (G["n9"][0], 0, (0, "mixed"), LM, 3),
    "rn10": (G["n10"][0], 0, (0, "mixed"), LM, 3),
    # 60 poses, one scene per kind, with false closures: rejected steps and accepted ones
    "r60_huber": (dict(n=60, n_closure=4, seed=6, drift=2.5, twice=False), 1, (ref.HUBER, "all"), LM, 6),
    "r60_cauchy": (dict(n=60, n_closure=4, seed=6, drift=1.5, twice=False), 1, (ref.CAUCHY, "all"), LM, 8),
    # (a drift of 3.5 gave more rejections but a start with |t| of 2.7e5: one rounding of the poses then moves
    # s = r^T Omega r by 2.4e-12 relative; test_sim3_robust_ref.py pins 1e-13 for every scene)
    "r60_gm": (dict(n=60, n_closure=4, seed=6, drift=1.5, twice=False), 2, (ref.GM, "closures"), LM, 5),
}
TRAJECTORY = tuple(SCENES)
SIXTY = ("r60_huber", "r60_cauchy", "r60_gm")


@functools.lru_cache(maxsize=None)
def scene(name):
    args, n_bad, kernel, _, _ = SCENES[name]
    g = sim3_cases.graph(**args)
    return with_kernels(corrupt(g, n_bad) if n_bad else g, *kernel)   # (kind, where[, scale])


def options(name, **over):
    kw = dict(SCENES[name][3], max_iter=SCENES[name][4])
    kw.update(over)
    return make_options(**kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(rows, converged, poses) of sim3_robust_ref.lm on the scene with its options; shared, read-only"""
    return ref.lm(scene(name), options(name))


@functools.lru_cache(maxsize=None)
def reference_cholesky(name):
    return ref.lm(scene(name), options(name), ref.solve_cholesky)


def exact_graph(kind):
    """exact Z at the truth, every pose at its truth: s = 0 up to rounding, so w == 1.0 for every kind"""
    g = sim3_cases.graph(n=12, n_closure=3, seed=11, exact=True, start_off=0.0, min_gap=3)
    return with_kernels(g, kind, "all", 1.0)
