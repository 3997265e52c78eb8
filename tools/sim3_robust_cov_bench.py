"""What the robust kernels, the covariance blocks and the gate of the Sim(3) graph cost (ba_sim3_*,
DESIGN.md §6p), on the three graphs of tools/sim3_graph_bench.py (§6o):

  (a) plain     the plain Sim(3) graph, per LM iteration: the figure to hold beside the parent
                commit's build (the same tool section runs on either: --plain-only);
  (b) cauchy    Cauchy on every factor beside it, and the ratio;
  (c) cov       ba_sim3_covariance for all poses and for 100 pairs, ba_sim3_gate for 100
                candidates, beside ba_pgraph_covariance / ba_pgraph_gate on the SE(3) graph of the
                same structure: wall time of the call with the stream idle before and after.

Device time of (a) and (b) from ba_sim3_last_ms (events around the enqueued loop), thresholds
negative so that every iteration runs; per repetition a fresh object, --warmup iterations, the
start values again, then --steps iterations; best of --reps.  From one instrumented pass the
time per launch of the graph's own kernels.

    python tools/sim3_robust_cov_bench.py [--out profiles/sim3_robust_cov_v1.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bundle_adjustment_solver_amd._lib import BaError, make_options  # noqa: E402
from bundle_adjustment_solver_amd.solver import ROBUST_CAUCHY, BaPoseGraph, BaSim3Graph  # noqa: E402

import pgo_cases  # noqa: E402
from sim3_graph_bench import GRAPHS, lifted  # noqa: E402


def solve_time(make, start, args, own=("k_s3_", "k_pg_control")):
    opt_w = make_options(max_iter=args.warmup, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4)
    opt = make_options(max_iter=args.steps, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4)
    times = []
    for _ in range(args.reps):
        p = make()
        p.solve(opt_w)
        p.update_values(start)
        p.solve(opt)
        times.append(p.last_ms() / args.steps)
        p.close()
    p = make()
    p._owner.enable_stage_timing(True)
    p._owner.get_kernel_ms(reset=True)
    p.solve(opt)
    km = p._owner.get_kernel_ms(reset=True)
    p._owner.enable_stage_timing(False)
    p.close()
    return times, {k: v for k, v in km.items() if v[1] and k.startswith(own)}


def call_time(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--no-cov", action="store_true", help="leave out (c)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["sim3_robust_cov_bench: %d + %d iterations, best of %d fresh objects" % (args.warmup, args.steps, args.reps)]
    for name, kw in GRAPHS:
        if args.only and name != args.only:
            continue
        g = pgo_cases.graph(**kw)
        S, fx, rels = lifted(g)
        F = len(rels["j"])
        try:
            plain, own = solve_time(lambda: BaSim3Graph(S, fx, rels), S, args)
        except BaError as e:   # the image does not fit
            lines.append("%-10s left out: %s" % (name, e))
            continue
        lines.append("%-10s (a) plain  %.4f ms / iteration (all %d: %s)"
                     % (name, min(plain), args.reps, " ".join("%.4f" % t for t in plain)))
        for k in sorted(own):
            lines.append("             %-22s %9.2f us / launch, %d launches" % (k, own[k][0] / own[k][1] * 1e3, own[k][1]))
        if args.plain_only:
            continue

        def robust():
            p = BaSim3Graph(S, fx, rels)
            p.set_robust(np.full(F, ROBUST_CAUCHY, np.int32), np.full(F, 30.0))
            return p
        rb, own = solve_time(robust, S, args)
        lines.append("%-10s (b) cauchy %.4f ms / iteration (all: %s), %.3f x plain"
                     % (name, min(rb), " ".join("%.4f" % t for t in rb), min(rb) / min(plain)))
        for k in sorted(own):
            lines.append("             %-22s %9.2f us / launch, %d launches" % (k, own[k][0] / own[k][1] * 1e3, own[k][1]))
        if args.no_cov:
            continue
        rng = np.random.default_rng(7)
        opt_idx = np.flatnonzero(np.asarray(fx) == 0)
        pj = rng.choice(opt_idx, 100)
        pk = np.array([int(rng.choice(opt_idx[opt_idx != j])) for j in pj])
        a = BaSim3Graph(S, fx, rels)
        b = BaPoseGraph(g["pose_T"], g["pose_fixed"], g["rels"])
        Z7 = np.tile(np.r_[np.eye(3).reshape(9), np.zeros(3), 1.0], (100, 1))
        Z6 = Z7[:, :12].copy()
        O7, O6 = np.tile(100.0 * np.eye(7), (100, 1, 1)), np.tile(100.0 * np.eye(6), (100, 1, 1))
        rows = [("covariance, all %d poses" % len(opt_idx), lambda: a.covariance(), lambda: b.covariance()),
                ("covariance, 100 pairs", lambda: a.covariance([], (pj, pk)), lambda: b.covariance([], (pj, pk))),
                ("gate, 100 candidates", lambda: a.gate(pj, pk, Z7, O7), lambda: b.gate(pj, pk, Z6, O6))]
        for what, f7, f6 in rows:
            t7, t6 = call_time(f7, args.reps), call_time(f6, args.reps)
            lines.append("%-10s (c) %-28s Sim(3) %9.3f ms  SE(3) %9.3f ms  ratio %.2f  (%d / %d batches)"
                         % (name, what, t7, t6, t7 / t6, a.cov_info()["batches"], b.cov_info()["batches"]))
        a.close()
        b.close()
        print("\n".join(lines), flush=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
