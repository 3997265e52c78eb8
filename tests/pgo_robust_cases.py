"""Seeded pose graphs with robust kernels and false closures (scaled units, no GPU), built on
pgo_cases.graph.  A graph here is the dict of pgo_cases with two more keys, kind (F,) and scale
(F,), which pgo_robust_ref reads.

corrupt(g, n_bad): the last n_bad factors (closures: pgo_cases appends them after the chain)
become false closures, in order, from one generator:
    rng = np.random.default_rng(5)
    Z <- compose(se3_exp(np.r_[5.0 * rng.standard_normal(3), 0.5 * rng.standard_normal(3)]), Z)

OUTLIERS: the two scenes of DESIGN.md §6l (40 poses with 2 false closures of 8, 70 poses with 3
of 10), the kernel on the closures only, scale 30, 12 iterations.
SCENES: the trajectory scenes the GPU is compared on: name -> (graph arguments, false closures,
kernel placement, option arguments, iterations).  The iteration counts are capped so that every
gain ratio of the reference stays clear of 0.25 and 0.5 and every iteration still moves the cost
(test_pgo_robust_ref.py pins both).
"""
import functools

import numpy as np

from bundle_adjustment_solver_amd._lib import make_options

import pgo_cases
import pgo_robust_ref as ref
from prior_ref import compose, se3_exp

SCALE = 30.0


def corrupt(g, n_bad, seed=5):
    rng = np.random.default_rng(seed)
    Z = np.array(g["rels"]["Z"], np.float64)
    F = Z.shape[0]
    for f in range(F - n_bad, F):
        Z[f] = compose(se3_exp(np.r_[5.0 * rng.standard_normal(3), 0.5 * rng.standard_normal(3)]), Z[f])
    return dict(g, rels=dict(g["rels"], Z=Z))


def closures(g):
    """the factors that are not chain factors (q + 1, q)"""
    j, k = np.asarray(g["rels"]["j"], np.int64), np.asarray(g["rels"]["k"], np.int64)
    return np.flatnonzero(j != k + 1)


def with_kernels(g, kind, where, scale=SCALE):
    """where: "closures", "all", "mixed" (kinds 0, 1, 2, 3 in turn over all factors, `kind`
    unused) or an index array"""
    F = len(g["rels"]["j"])
    kd = np.zeros(F, np.int32)
    if isinstance(where, str) and where == "mixed":
        kd[:] = np.arange(F) % 4
    elif isinstance(where, str) and where == "all":
        kd[:] = kind
    elif isinstance(where, str) and where == "closures":
        kd[closures(g)] = kind
    else:
        kd[np.asarray(where, np.int64)] = kind
    return dict(g, kind=kd, scale=np.full(F, float(scale)))


def without_factors(g, drop):
    keep = np.setdiff1d(np.arange(len(g["rels"]["j"])), drop)
    return dict(g, rels={key: np.asarray(v)[keep] for key, v in g["rels"].items()})


LM = dict(thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4)
# name -> (graph arguments, false closures); the recipe of the issue that asked for the kernels
OUTLIERS = {
    "o40": (dict(n=40, n_closure=8, seed=21, drift=0.03, twice=False), 2),
    "o70": (dict(n=70, n_closure=10, seed=33, drift=0.1, twice=False), 3),
}
OUTLIER_ITERATIONS = 12


@functools.lru_cache(maxsize=None)
def outlier_scene(name):
    """-> (corrupted graph without kernels, indices of the false closures, the inlier closures)"""
    args, n_bad = OUTLIERS[name]
    g = corrupt(pgo_cases.graph(**args), n_bad)
    F = len(g["rels"]["j"])
    bad = np.arange(F - n_bad, F)
    return g, bad, np.setdiff1d(closures(g), bad)


def outlier_options():
    return make_options(max_iter=OUTLIER_ITERATIONS, **LM)


@functools.lru_cache(maxsize=None)
def outlier_clean(name):
    """poses of the non-robust solve with the false closures removed"""
    g, bad, _ = outlier_scene(name)
    return ref.lm(without_factors(g, bad), outlier_options())[2]


@functools.lru_cache(maxsize=None)
def outlier_reference(name, kind, cholesky=False):
    """(rows, converged, poses) of the reference with `kind` on the closures (0: none)"""
    g = outlier_scene(name)[0]
    g = with_kernels(g, kind, "closures") if kind else g
    return ref.lm(g, outlier_options(), ref.solve_cholesky if cholesky else ref.solve_numpy)


# name -> (graph arguments, false closures, (kind, where), option arguments, iterations)
# The r40 scenes are the 40-pose outlier scene (rho turns to noise after 4 to 6 iterations at
# its drift of 0.03); the r60 scenes are the 63 / 64 / 65-factor graphs of pgo_cases with false
# closures and a drift raised until the reference rejects steps: r60_huber, r60_cauchy and
# r60_gm each hold decisive rejections followed by decisive accepted steps.
SCENES = {
    "r40_huber": (OUTLIERS["o40"][0], 2, (ref.HUBER, "closures"), LM, 5),
    "r40_cauchy": (OUTLIERS["o40"][0], 2, (ref.CAUCHY, "closures"), LM, 4),
    "r40_gm": (OUTLIERS["o40"][0], 2, (ref.GM, "closures"), LM, 6),
    "r60_huber": (dict(n=60, n_closure=3, seed=6, drift=0.8), 1, (ref.HUBER, "all"), LM, 10),       # 63 factors
    "r60_mixed": (dict(n=60, n_closure=4, seed=7, drift=2.5), 1, (0, "mixed"), LM, 8),               # 64
    "r60_cauchy": (dict(n=60, n_closure=5, seed=8, drift=1.5), 2, (ref.CAUCHY, "all"), LM, 10),      # 65
    "r60_gm": (dict(n=60, n_closure=5, seed=8, drift=2.5), 2, (ref.GM, "closures"), LM, 9),          # 65
    # N = 5, 6, 10, 11 optimisable poses (the pose-per-tile edges), 1 optimisable pose
    "rn5": (pgo_cases.SCENES["n5"][0], 1, (0, "mixed"), LM, 3),
    "rn6": (pgo_cases.SCENES["n6"][0], 1, (0, "mixed"), LM, 3),
    "rn10": (pgo_cases.SCENES["n10"][0], 1, (0, "mixed"), LM, 3),
    "rn11": (pgo_cases.SCENES["g12"][0], 1, (0, "mixed"), LM, 3),
    "r2": (dict(n=2, seed=1, drift=0.5), 0, (ref.CAUCHY, "all", 1.0), LM, 2),
}
TRAJECTORY = tuple(SCENES)


@functools.lru_cache(maxsize=None)
def scene(name):
    args, n_bad, kernel, _, _ = SCENES[name]
    g = pgo_cases.graph(**args)
    return with_kernels(corrupt(g, n_bad) if n_bad else g, *kernel)   # (kind, where[, scale])


def options(name, **over):
    kw = dict(SCENES[name][3], max_iter=SCENES[name][4])
    kw.update(over)
    return make_options(**kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(rows, converged, poses) of pgo_robust_ref.lm on the scene with its options; shared, read-only"""
    return ref.lm(scene(name), options(name))


@functools.lru_cache(maxsize=None)
def reference_cholesky(name):
    return ref.lm(scene(name), options(name), ref.solve_cholesky)
