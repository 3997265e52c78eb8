"""Time per LM iteration of the Sim(3) pose-graph optimisation (ba_sim3_*) beside
the SE(3) graph (ba_pgraph_*, §6k) on the same structure, measured in the same process:

  chain1000   a chain of 1 000 poses;
  loops1000   the same chain plus 100 loop closures at least 100 poses apart;
  loops5000   5 000 poses with 500 closures (if the image fits).

The graphs are those of tools/pose_graph_bench.py (tests/pgo_cases.py), lifted to similarities:
every pose and measurement with scale 1, Omega = diag(Omega_6x6, the mean of its rotation
diagonal) for sigma; one fixed pose.  The Sim(3) image has 7 / 6 of the columns and 4 / 9 poses per
tile where the SE(3) image has 5 / 10, so its time is expected above the SE(3) time: the ratio is
reported, nothing is tuned for it.

Device time from ba_sim3_last_ms / ba_pgraph_last_ms (events around the enqueued loop),
thresholds negative so that every iteration runs; per repetition a fresh object, --warmup
iterations, the start values again (update_values), then --steps iterations; best of --reps.
From one instrumented pass (ba_get_kernel_ms on the borrowed handle) the split between the dense
solve (k_dense_init and the k_chol_* kernels) and the graph's own kernels (k_s3_* and
k_pg_control; k_pg_* for the SE(3) graph).

    python tools/sim3_graph_bench.py [--out profiles/sim3_graph_v1.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bundle_adjustment_solver_amd._lib import BaError, make_options  # noqa: E402
from bundle_adjustment_solver_amd.solver import BaPoseGraph, BaSim3Graph  # noqa: E402

import pgo_cases  # noqa: E402

GRAPHS = (("chain1000", dict(n=1000, n_closure=0, seed=21)),
          ("loops1000", dict(n=1000, n_closure=100, seed=21, min_gap=100)),
          ("loops5000", dict(n=5000, n_closure=500, seed=22, min_gap=100)))


def lifted(g):
    """the SE(3) graph as similarities: (pose_S, pose_fixed, rels)"""
    F = len(g["rels"]["j"])
    Om6 = np.asarray(g["rels"]["Omega"], np.float64).reshape(F, 6, 6)
    Om = np.zeros((F, 7, 7))
    Om[:, :6, :6] = Om6
    Om[:, 6, 6] = Om6[:, [3, 4, 5], [3, 4, 5]].mean(axis=1)
    rels = dict(j=g["rels"]["j"], k=g["rels"]["k"], Z=np.c_[g["rels"]["Z"], np.ones(F)], Omega=Om)
    return np.c_[g["pose_T"], np.ones(len(g["pose_T"]))], g["pose_fixed"], rels


def measure(make, own, args):
    """make() -> (object, start values); own: the prefixes of the graph's own kernels"""
    opt_w = make_options(max_iter=args.warmup, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4)
    opt = make_options(max_iter=args.steps, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4)
    best, info, rows = None, None, None
    for _ in range(args.reps):
        p, start = make()
        p.solve(opt_w)
        p.update_values(start)
        rows, _ = p.solve(opt)
        ms = p.last_ms() / args.steps
        best = ms if best is None else min(best, ms)
        info = p.info()
        p.close()
    p, _ = make()   # one instrumented pass: where the time goes
    p._owner.enable_stage_timing(True)
    p._owner.get_kernel_ms(reset=True)
    p.solve(opt)
    km = p._owner.get_kernel_ms(reset=True)
    p._owner.enable_stage_timing(False)
    p.close()
    dense = sum(v[0] for k, v in km.items() if k.startswith("k_chol_") or k == "k_dense_init") / args.steps
    mine = {k: v for k, v in km.items() if v[1] and k.startswith(own)}
    return best, info, rows, dense, mine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["sim3_graph_bench: %d + %d iterations, best of %d fresh objects, device time of ba_sim3_last_ms / "
             "ba_pgraph_last_ms" % (args.warmup, args.steps, args.reps)]
    for name, kw in GRAPHS:
        if args.only and name != args.only:
            continue
        g = pgo_cases.graph(**kw)
        S, fx, rels = lifted(g)
        res = {}
        try:
            res["sim3"] = measure(lambda: (BaSim3Graph(S, fx, rels), S), ("k_s3_", "k_pg_control"), args)
            res["se3"] = measure(lambda: (BaPoseGraph(g["pose_T"], g["pose_fixed"], g["rels"]), g["pose_T"]),
                                 ("k_pg_",), args)
        except BaError as e:   # the image does not fit
            lines.append("%-10s left out: %s" % (name, e))
            print(lines[-1], flush=True)
            continue
        for kind in ("sim3", "se3"):
            ms, info, rows, dense, mine = res[kind]
            st = [r.iteration_status for r in rows]
            own_ms = sum(v[0] for v in mine.values()) / args.steps
            lines.append("%-10s %-4s %5d poses %5d factors  GPU %.4f ms / iteration  tiles %d x nb%d  levels %d  image %.1f "
                         "MiB  pivots %d  statuses 0/1/2 %d/%d/%d  chi2 %.4e -> %.4e"
                         % (name, kind, len(fx), info["factors"], ms, info["tiles"], info["nb"], info["levels"],
                            info["image_bytes"] / 2 ** 20, info["bad_pivots"], st.count(0), st.count(1), st.count(2),
                            rows[0].trial_cost, rows[-1].cost))
            lines.append("           instrumented pass, per iteration: dense solve %.4f ms, the graph's own kernels %.4f ms"
                         % (dense, own_ms))
            for k in sorted(mine):
                lines.append("             %-16s %9.2f us / launch, %d launches" % (k, mine[k][0] / mine[k][1] * 1e3, mine[k][1]))
        lines.append("           Sim(3) / SE(3): %.2f x per iteration, dense solve %.2f x"
                     % (res["sim3"][0] / res["se3"][0], res["sim3"][3] / max(res["se3"][3], 1e-12)))
        print("\n".join(lines[-1:]), flush=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
