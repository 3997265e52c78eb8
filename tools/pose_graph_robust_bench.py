"""Cost of the robust kernels of the pose-graph optimisation (ba_pgraph_set_robust, DESIGN.md
§6l): time per LM iteration on the three graphs of tools/pose_graph_bench.py (chain1000,
loops1000, loops5000) in three configurations:

  none      no kernel: the plain k_pg_lin / k_pg_assemble, the figure pose_graph_bench.py reports;
  closures  Cauchy (scale 30) on the loop closures only (the chain has none: the plain kernels);
  all       Cauchy on every factor.

The protocol is pose_graph_bench.py's: device time from ba_pgraph_last_ms, thresholds negative,
per repetition a fresh object, --warmup iterations, the start values again, then --steps
iterations; best of --reps.  From one instrumented pass the time of the dense solve and of the
k_pg_* kernels, and the k_pg_* share of their sum.

    python tools/pose_graph_robust_bench.py [--configs none,closures,all] [--out profiles/pose_graph_robust_v1.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bundle_adjustment_solver_amd._lib import make_options  # noqa: E402
from bundle_adjustment_solver_amd.solver import ROBUST_CAUCHY, BaPoseGraph  # noqa: E402

import pgo_cases  # noqa: E402
from pose_graph_bench import GRAPHS  # noqa: E402

SCALE = 30.0


def kinds(g, config):
    j, k = np.asarray(g["rels"]["j"], np.int64), np.asarray(g["rels"]["k"], np.int64)
    kd = np.zeros(len(j), np.int32)
    if config == "closures":
        kd[j != k + 1] = ROBUST_CAUCHY
    elif config == "all":
        kd[:] = ROBUST_CAUCHY
    return kd


def make(g, kd):
    p = BaPoseGraph(g["pose_T"], g["pose_fixed"], g["rels"])
    if kd.any():   # "none" never calls set_robust: the object of pose_graph_bench.py
        p.set_robust(kd, np.full(len(kd), SCALE))
    return p


def measure(g, kd, args):
    opt_w = make_options(max_iter=args.warmup, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4)
    opt = make_options(max_iter=args.steps, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4)
    runs, rows = [], None
    for _ in range(args.reps):
        p = make(g, kd)
        p.solve(opt_w)
        p.update_values(g["pose_T"])
        rows, _ = p.solve(opt)
        runs.append(p.last_ms() / args.steps)
        p.close()
    p = make(g, kd)   # one instrumented pass: where the time goes
    p._owner.enable_stage_timing(True)
    p._owner.get_kernel_ms(reset=True)
    p.solve(opt)
    km = p._owner.get_kernel_ms(reset=True)
    p._owner.enable_stage_timing(False)
    _, w = p.factor_report()
    p.close()
    return runs, rows, km, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--configs", default="none,closures,all")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["pose_graph_robust_bench: %d + %d iterations, best of %d fresh objects, device time of ba_pgraph_last_ms; "
             "Cauchy, scale %g" % (args.warmup, args.steps, args.reps, SCALE)]
    for name, kw in GRAPHS:
        if args.only and name != args.only:
            continue
        g = pgo_cases.graph(**kw)
        base = None
        for config in args.configs.split(","):
            kd = kinds(g, config)
            runs, rows, km, w = measure(g, kd, args)
            ms = min(runs)
            base = ms if config == "none" else base
            st = [r.iteration_status for r in rows]
            dense = sum(v[0] for k, v in km.items() if k.startswith("k_chol_") or k == "k_dense_init") / args.steps
            pg = sum(v[0] for k, v in km.items() if k.startswith("k_pg_")) / args.steps
            lines.append("%-10s %-8s %5d robust of %5d factors  GPU %.4f ms / iteration%s  (runs %s)  statuses 0/1/2 "
                         "%d/%d/%d  cost %.4e -> %.4e  weights %.3g .. %.3g"
                         % (name, config, int((kd != 0).sum()), len(kd), ms,
                            "" if base is None or config == "none" else "  %+.2f %% on none" % (100.0 * (ms / base - 1.0)),
                            " ".join("%.4f" % r for r in runs), st.count(0), st.count(1), st.count(2),
                            rows[0].trial_cost, rows[-1].cost, w.min(), w.max()))
            lines.append("           instrumented pass, per iteration: dense solve %.4f ms, k_pg_* %.4f ms (%.2f %% of both)"
                         % (dense, pg, 100.0 * pg / (dense + pg)))
            for k in sorted(km):
                if km[k][1] and k.startswith("k_pg_"):
                    lines.append("             %-22s %9.2f us / launch, %d launches"
                                 % (k, km[k][0] / km[k][1] * 1e3, km[k][1]))
            print("\n".join(lines[-2:]), flush=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
