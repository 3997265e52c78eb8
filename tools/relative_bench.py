"""Cost of relative-pose factors on the handle path (ba_set_relative) at BASELINE config C4
(1 000 poses / 500 k landmarks / 5 M observations), three ways:

  none     the handle without factors: what bench.py's headline measures;
  chain    the odometry chain (q + 1, q) over the optimisable poses;
  loops    the chain plus 100 loop closures between poses at least 100 apart (seeded).

Z = the relative pose of the start values moved by a 1e-2 tangent, Omega = J^T J of a seeded
random J scaled to the problem's A blocks (the factors of the tests, rel_ref.random_relatives
restated without the oracle).  Time per LM iteration as bench.py takes it: --warmup iterations,
then --steps iterations between two synchronisations, thresholds negative so that every
iteration runs; best of --reps, each from the start values.  For every run the dense schedule
(fill, levels: loop closures add fill to the factor) and, from one instrumented pass, the
per-launch time of the three k_rel_* kernels (ba_get_kernel_ms).

    python tools/relative_bench.py [--config C4] [--out profiles/relative_v1.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bundle_adjustment_solver_amd import scenes  # noqa: E402
from bundle_adjustment_solver_amd._lib import make_options  # noqa: E402
from bundle_adjustment_solver_amd.solver import BaProblem  # noqa: E402


def se3_exp(xi):
    v, w = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        R, V = np.eye(3) + K, np.eye(3) + 0.5 * K
    else:
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    return R, V @ v


def factors(pr, pairs, seed, scale):
    rng = np.random.default_rng(seed)
    T = np.asarray(pr["pose_T"], np.float64)
    d = np.r_[np.ones(3), np.full(3, 0.1)]
    F = len(pairs)
    Z, Om = np.zeros((F, 12)), np.zeros((F, 6, 6))
    for f, (j, k) in enumerate(pairs):
        Rj, tj = T[j, :9].reshape(3, 3), T[j, 9:]
        Rk, tk = T[k, :9].reshape(3, 3), T[k, 9:]
        RE = Rj @ Rk.T
        tE = tj - RE @ tk
        dR, dt = se3_exp(1e-2 * rng.standard_normal(6) / np.sqrt(6))
        Z[f, :9] = (dR @ RE).reshape(9)
        Z[f, 9:] = dR @ tE + dt
        J = rng.standard_normal((8, 6)) * scale * 0.3 * d[None, :]
        Om[f] = J.T @ J
    return dict(j=np.array([p[0] for p in pairs], np.int32), k=np.array([p[1] for p in pairs], np.int32), Z=Z,
                Omega=Om)


def make(pr, rels):
    p = BaProblem(0)
    p.set_cameras(pr["cam_intr"], pr["cam_T"])
    p.set_poses(pr["pose_T"], pr["pose_fixed"])
    p.set_points(pr["pt_X"], pr["pt_fixed"])
    p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
    if rels is not None:
        p.set_relative(rels)
    p.finalize()
    return p


def measure(p, pr, args):
    opt = make_options(max_iter=args.warmup + args.steps + 1, thr_step=-1.0, thr_cost=-1.0)
    best = None
    for _ in range(args.reps):
        p.update_values(pr["pose_T"], pr["pt_X"])
        p.lm_begin(opt)
        p.lm_iterate(args.warmup)
        p.lm_sync()
        t0 = time.perf_counter()
        p.lm_iterate(args.steps)
        p.lm_sync()
        ms = (time.perf_counter() - t0) / args.steps * 1e3
        best = ms if best is None else min(best, ms)
    # one instrumented pass: per-launch time of the factor kernels
    p.update_values(pr["pose_T"], pr["pt_X"])
    p.enable_stage_timing(True)
    p.get_kernel_ms(reset=True)
    p.lm_begin(opt)
    p.lm_iterate(args.steps)
    p.lm_sync()
    km = p.get_kernel_ms(reset=True)
    p.enable_stage_timing(False)
    rel = {k: (v[0] / max(v[1], 1) * 1e3, v[1]) for k, v in km.items() if k.startswith("k_rel_")}
    return best, rel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pr = scenes.scaled_problem(scenes.config_scene(args.config))
    fixed = np.asarray(pr["pose_fixed"]) != 0
    opt_poses = np.flatnonzero(~fixed)
    # the scale of the problem's own A blocks, from a handle without factors
    p = make(pr, None)
    p.stage_linearize(0.0, 1.0)
    scale = float(np.sqrt(np.abs(p.get_A()[0]).max()))
    chain = [(int(opt_poses[q + 1]), int(opt_poses[q])) for q in range(len(opt_poses) - 1)]
    rng = np.random.default_rng(9)
    loops = []
    while len(loops) < 100 and len(opt_poses) > 101:
        a, b = (int(x) for x in rng.choice(opt_poses, 2, replace=False))
        if abs(a - b) >= 100:
            loops.append((a, b))
    lines = ["relative_bench: %s, %d poses (%d optimisable), %d observations, %d + %d iterations, best of %d"
             % (args.config, len(fixed), len(opt_poses), len(pr["obs_cam"]), args.warmup, args.steps, args.reps)]
    base = None
    for name, pairs in (("none", None), ("chain", chain), ("loops", chain + loops)):
        if pairs is not None:
            p.close()
            p = make(pr, factors(pr, pairs, 5, scale))
        ms, rel = measure(p, pr, args)
        base = ms if base is None else base
        di, ri = p.get_dense_info(), p.relative_info()
        lines.append("%-6s %4d factors  %.4f ms / iteration (%+.1f %%)  dense fill %.4f levels %d npad %d  "
                     "coupled blocks %d (only from a factor %d)  %d B"
                     % (name, ri["factors"], ms, (ms / base - 1) * 100, di["fill"], di["levels"], di["npad"],
                        ri["blocks"], ri["blocks_only"], ri["bytes"]))
        for k in sorted(rel):
            lines.append("         %-14s %.2f us / launch, %d launches" % (k, rel[k][0], rel[k][1]))
    p.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
