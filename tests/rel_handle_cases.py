"""The scenes and factor sets shared by the CPU and GPU tests of the relative-pose factors on
the handle path (ba_set_relative).  Host only: numpy and the CPU oracle."""
import functools

import numpy as np

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import make_options
from oracle import oracle_py as O

import rel_ref

ITERS = 8
SEED = 5
STRENGTH = 3.0
BLIND = 17   # the pose of the 30-pose scene whose observations are removed in the "blind" case


def factor_pairs(pr):
    """the chain (q + 1, q) from the last fixed pose on; four far pairs, two in each
    orientation; one factor with j fixed and one with k fixed; one pair named twice, in
    opposite orientations"""
    fixed = np.asarray(pr["pose_fixed"]) != 0
    n = len(fixed)
    fx = np.flatnonzero(fixed)
    assert len(fx) and (fx == np.arange(len(fx))).all(), "the scenes fix their first poses"
    o = np.flatnonzero(~fixed)
    last = int(fx[-1])
    pairs = [(q + 1, q) for q in range(last, n - 1)]
    pairs += [(int(o[-2]), int(o[1])), (int(o[2]), int(o[-1])), (int(o[-4]), int(o[len(o) // 3])),
              (int(o[len(o) // 4]), int(o[-6]))]
    pairs += [(int(fx[0]), int(o[3])), (int(o[4]), int(fx[0]))]
    pairs += [(int(o[5]), int(o[7])), (int(o[7]), int(o[5]))]
    return pairs


def without_pose(pr, pose):
    """the problem without any observation of `pose`"""
    keep = np.asarray(pr["obs_pose"]) != pose
    out = dict(pr)
    for key in ("obs_cam", "obs_pose", "obs_pt"):
        out[key] = np.ascontiguousarray(np.asarray(pr[key])[keep])
    out["obs_uv"] = np.ascontiguousarray(np.asarray(pr["obs_uv"]).reshape(-1, 2)[keep])
    return out


SCENES = {
    "group150": lambda: scenes.scaled_problem(scenes.synthetic_ba_scene(150, 9000, 5, True, seed=33, pixel_sigma=0.3)),
    "chunk60": lambda: scenes.scaled_problem(scenes.test_ba_scene()),
    "small30": lambda: scenes.scaled_problem(scenes.synthetic_ba_scene(30, 600, 5, True, 3)),
    "blind30": lambda: without_pose(scenes.scaled_problem(scenes.synthetic_ba_scene(30, 600, 5, True, 3)), BLIND),
}
# name -> options of the parity run (thresholds off, 8 iterations; the chunk scene also once
# in Gauss-Newton mode, see GN below)
LM = dict(max_iter=ITERS, thr_step=0.0, thr_cost=0.0)
GN = dict(max_iter=4, thr_step=0.0, thr_cost=0.0, lambda0=1e-3, gauss_newton=True)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (problem, factors): computed once per process and shared — do not modify"""
    pr = SCENES[name]()
    # the factors of the blind scene are those of the full one: Z and Omega do not depend on
    # the observations that were removed
    base = SCENES["small30"]() if name == "blind30" else pr
    rels = rel_ref.random_relatives(base, factor_pairs(base), seed=SEED, strength=STRENGTH)
    return pr, rels


@functools.lru_cache(maxsize=None)
def reference(name, gn=False):
    """-> (rows, converged, poses, points) of rel_ref.lm_with_relatives; shared, do not modify"""
    pr, rels = case(name)
    return rel_ref.lm_with_relatives(pr, rels, make_options(**(GN if gn else LM)))


@functools.lru_cache(maxsize=None)
def plain_oracle_rows(name):
    """the rows of the oracle's own loop on the problem without factors"""
    pr, _ = case(name)
    o = O.Oracle(pr)
    rows, _ = o.solve(O.make_options(**LM))
    o.close()
    return rows
