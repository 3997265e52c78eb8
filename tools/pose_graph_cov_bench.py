"""Time of the pose graph's covariance blocks and chi-square gate (ba_pgraph_covariance /
ba_pgraph_gate) on the three seeded graphs of tools/pose_graph_bench.py, every
one with one fixed pose, at their start poses:

  chain1000   a chain of 1 000 poses;
  loops1000   the same chain plus 100 loop closures at least 100 poses apart;
  loops5000   5 000 poses with 500 closures.

Per graph: all pose blocks; 1 000 candidates against the newest pose (each one a wave of its
own); the empty selection, which is the factorisation alone.  GPU: events on the handle's
stream around the call, so the figure includes the call's uploads, its synchronisations and the
download of the blocks; one warm-up call, best of --reps.  Host route: BaPoseGraph.system()
(a dense download) plus numpy.linalg.inv, wall clock, once; skipped above --host-max poses
(6N x 6N doubles: 7.2 GB at 5 000 poses).

    python tools/pose_graph_cov_bench.py [--out profiles/pose_graph_cov_v1.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bundle_adjustment_solver_amd.solver import BaPoseGraph, BaProblem  # noqa: E402

import pgo_cases  # noqa: E402
import rel_ref  # noqa: E402
from pose_graph_bench import GRAPHS  # noqa: E402
from prior_ref import compose  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--only", default=None)
    ap.add_argument("--host-max", type=int, default=1000, help="largest graph (poses) for the host route")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
    lines = ["pose_graph_cov_bench: events on the stream around the call, one warm-up call, best of %d" % a.reps]

    def timed(call):
        best, out = None, None
        for rep in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = call()
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if rep > 0:
                best = ms if best is None else min(best, ms)
        return best, out

    for name, kw in GRAPHS:
        if a.only and name != a.only:
            continue
        g = pgo_cases.graph(**kw)
        n = len(g["pose_fixed"])
        owner = BaProblem(0)
        owner.set_stream(stream.cuda_stream)
        p = BaPoseGraph(g["pose_T"], g["pose_fixed"], g["rels"], owner=owner)
        info = p.info()
        lines.append("%-10s %5d poses %5d factors  tiles %d x nb%d  levels %d  image %.1f MiB"
                     % (name, n, info["factors"], info["tiles"], info["nb"], info["levels"], info["image_bytes"] / 2 ** 20))
        ms_all, (cp, _, _) = timed(lambda: p.covariance())
        ci = p.cov_info()
        lines.append("  all %d pose blocks: %.3f ms, %d batch(es) of %d columns (workspace %.0f MiB), dropped pivots %d"
                     % (len(cp), ms_all, ci["batches"], ci["batch_cols"], ci["workspace_bytes"] / 2 ** 20, p.dropped_pivots))
        rng = np.random.default_rng(1)
        ck = rng.integers(0, n - 1, a.candidates).astype(np.int32)
        cj = np.full(a.candidates, n - 1, np.int32)
        T = g["pose_T"]
        Z = np.array([compose(T[n - 1], rel_ref.inverse12(T[k])) for k in ck])
        Om = np.tile(100.0 * np.eye(6), (a.candidates, 1, 1))
        ms_gate, (d2, _, _) = timed(lambda: p.gate(cj, ck, Z, Om))
        ci = p.cov_info()
        lines.append("  %d candidates against pose %d: %.3f ms, %d batch(es); d2 of a candidate at the estimate itself "
                     "<= %.2e" % (a.candidates, n - 1, ms_gate, ci["batches"], np.abs(d2).max()))
        ms_0, _ = timed(lambda: p.covariance([], None))
        lines.append("  empty selection (linearise + assemble + factorise only): %.3f ms" % ms_0)
        if n <= a.host_max:
            t0 = time.perf_counter()
            H, _ = p.system()
            t1 = time.perf_counter()
            S = np.linalg.inv(H)
            t2 = time.perf_counter()
            diag = np.array([S[6 * q:6 * q + 6, 6 * q:6 * q + 6] for q in range(len(cp))])
            err = (np.abs(cp - diag).reshape(len(cp), -1).max(axis=1) / np.abs(diag).reshape(len(cp), -1).max(axis=1)).max()
            lines.append("  host route: system() %.1f ms + numpy.linalg.inv %.1f ms = %.1f ms (%.0f x the GPU's all-blocks "
                         "call); largest relative block difference %.2e"
                         % ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3, (t2 - t0) * 1e3 / ms_all, err))
        else:
            lines.append("  host route: skipped (%d x %d doubles)" % (6 * (n - 1), 6 * (n - 1)))
        p.close()
        owner.close()
        print("\n".join(lines[-5:]), flush=True)
    text = "\n".join(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
