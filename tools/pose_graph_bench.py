"""Time per LM iteration of the pose-graph optimisation (ba_pgraph_*) on three
seeded graphs of tests/pgo_cases.py, every one with one fixed pose:

  chain1000   a chain of 1 000 poses;
  loops1000   the same chain plus 100 loop closures at least 100 poses apart;
  loops5000   5 000 poses with 500 closures.

GPU: device time from ba_pgraph_last_ms (events around the enqueued loop), thresholds negative
so that every iteration runs; per repetition a fresh object, --warmup iterations, the start
values again (update_values), then --steps iterations; best of --reps.  From one instrumented
pass (ba_get_kernel_ms on the borrowed handle) the split between the dense solve (k_dense_init
and the k_chol_* kernels) and the four k_pg_* kernels.

Host: the same iteration (tests/pgo_ref.py: chi-square LM) with the system assembled as sparse
6x6 blocks and scipy.sparse.linalg.spsolve for the step, one iteration timed, best of 2.

    python tools/pose_graph_bench.py [--out profiles/pose_graph_v1.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse
import scipy.sparse.linalg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bundle_adjustment_solver_amd._lib import make_options  # noqa: E402
from bundle_adjustment_solver_amd.solver import BaPoseGraph, relative_residual  # noqa: E402

import pgo_cases  # noqa: E402
import pgo_ref  # noqa: E402
import rel_ref  # noqa: E402
from prior_ref import compose, sym_lower  # noqa: E402

GRAPHS = (("chain1000", dict(n=1000, n_closure=0, seed=21)),
          ("loops1000", dict(n=1000, n_closure=100, seed=21, min_gap=100)),
          ("loops5000", dict(n=5000, n_closure=500, seed=22, min_gap=100)))


def host_iteration(g, lam):
    """one iteration of pgo_ref.lm with sparse blocks and spsolve -> (seconds, chi2 before, after)"""
    T, rels = np.asarray(g["pose_T"], np.float64), g["rels"]
    jopt = rel_ref.opt_index(dict(pose_fixed=g["pose_fixed"]))
    N = int((jopt >= 0).sum())
    t0 = time.perf_counter()
    rows, cols, vals = [], [], []
    gr = np.zeros(6 * N)
    blk = np.arange(6)
    rr, cc = np.repeat(blk, 6), np.tile(blk, 6)
    chi0 = 0.0
    for f in range(len(rels["j"])):
        j, k = int(rels["j"][f]), int(rels["k"][f])
        r = relative_residual(T[j], T[k], rels["Z"][f])
        Om = sym_lower(rels["Omega"][f])
        chi0 += r @ Om @ r
        Ad = rel_ref.adjoint(compose(T[j], rel_ref.inverse12(T[k])))
        a, b = jopt[j], jopt[k]
        OA = Om @ Ad

        def put(p, q, M):
            rows.append(6 * p + rr)
            cols.append(6 * q + cc)
            vals.append(M.reshape(-1))

        if a >= 0:
            put(a, a, Om)
            gr[6 * a:6 * a + 6] += -Om @ r
        if b >= 0:
            put(b, b, Ad.T @ OA)
            gr[6 * b:6 * b + 6] += Ad.T @ (Om @ r)
        if a >= 0 and b >= 0:
            put(a, b, -OA)
            put(b, a, -OA.T)
    H = scipy.sparse.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))),
                                shape=(6 * N, 6 * N)).tocsc()
    d = H.diagonal()
    x = scipy.sparse.linalg.spsolve(H + lam * scipy.sparse.diags(d), gr)
    Tt = pgo_ref.moved(T, x, np.flatnonzero(jopt >= 0))
    chi1 = pgo_ref.chi2(Tt, rels)
    return time.perf_counter() - t0, chi0, chi1


def measure(g, args):
    opt_w = make_options(max_iter=args.warmup, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4)
    opt = make_options(max_iter=args.steps, thr_step=-1.0, thr_cost=-1.0, lambda0=1e-4)
    best, info, rows = None, None, None
    for _ in range(args.reps):
        p = BaPoseGraph(g["pose_T"], g["pose_fixed"], g["rels"])
        p.solve(opt_w)
        p.update_values(g["pose_T"])
        rows, _ = p.solve(opt)
        ms = p.last_ms() / args.steps
        best = ms if best is None else min(best, ms)
        info = p.info()
        p.close()
    # one instrumented pass: where the time goes
    p = BaPoseGraph(g["pose_T"], g["pose_fixed"], g["rels"])
    p._owner.enable_stage_timing(True)
    p._owner.get_kernel_ms(reset=True)
    p.solve(opt)
    km = p._owner.get_kernel_ms(reset=True)
    p._owner.enable_stage_timing(False)
    p.close()
    return best, info, rows, km


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["pose_graph_bench: %d + %d iterations, best of %d fresh objects, device time of ba_pgraph_last_ms"
             % (args.warmup, args.steps, args.reps)]
    for name, kw in GRAPHS:
        if args.only and name != args.only:
            continue
        g = pgo_cases.graph(**kw)
        ms, info, rows, km = measure(g, args)
        st = [r.iteration_status for r in rows]
        lines.append("%-10s %5d poses %5d factors  GPU %.4f ms / iteration  tiles %d x nb%d  levels %d  image %.1f MiB  "
                     "pivots %d  statuses 0/1/2 %d/%d/%d  chi2 %.4e -> %.4e"
                     % (name, len(g["pose_fixed"]), info["factors"], ms, info["tiles"], info["nb"], info["levels"],
                        info["image_bytes"] / 2 ** 20, info["bad_pivots"], st.count(0), st.count(1), st.count(2),
                        rows[0].trial_cost, rows[-1].cost))
        dense = sum(v[0] for k, v in km.items() if k.startswith("k_chol_") or k == "k_dense_init")
        pg = sum(v[0] for k, v in km.items() if k.startswith("k_pg_"))
        lines.append("           instrumented pass, per iteration: dense solve %.4f ms, k_pg_* %.4f ms"
                     % (dense / args.steps, pg / args.steps))
        for k in sorted(km):
            if km[k][1] and (k.startswith("k_pg_") or k.startswith("k_chol_") or k == "k_dense_init"):
                lines.append("             %-16s %9.2f us / launch, %d launches" % (k, km[k][0] / km[k][1] * 1e3, km[k][1]))
        if not args.no_host:
            hs = min(host_iteration(g, 1e-4)[0] for _ in range(2))
            lines.append("           host (numpy blocks + scipy spsolve): %.1f ms / iteration  (%.0f x the GPU's)"
                         % (hs * 1e3, hs * 1e3 / ms))
        print("\n".join(lines[-2:]), flush=True)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
