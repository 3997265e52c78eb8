"""Batched full BA (ba_batch_solve, one workgroup per window) against the loop of
handles it replaces: B windows of 10 poses / ~300 landmarks, stereo, sigma = 0.5 px,
10 LM iterations (thresholds 0, so every window runs all of them).

Both sides are timed with hipEvents on the stream the work runs on, best of 5 after
one warm-up; planning (ba_batch_create / ba_finalize) is excluded from both and
reported separately.  The loop side is what a caller had before the batch existed: one
BaProblem per window, update_values + solve each.

    python tools/full_batch_bench.py [--B 64 1000] [--out profiles/full_batch_v1.txt]
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
from bundle_adjustment_solver_amd.solver import BaBatch, BaProblem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 1000])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=16,
                    help="distinct windows generated; the batch cycles through them")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
    opt = make_options(max_iter=a.iters, thr_step=0.0, thr_cost=0.0)
    base = [scenes.scaled_problem(s) for s in
            scenes.ba_batch_scene(a.distinct, n_pose=10, n_pt=300, stereo=True, pixel_sigma=0.5)]
    lines = []

    def timed(fn):
        best = float("inf")
        for r in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r > 0:
                best = min(best, e0.elapsed_time(e1))
        return best

    for B in a.B:
        probs = [base[k % len(base)] for k in range(B)]
        T0 = np.concatenate([p["pose_T"] for p in probs])
        X0 = np.concatenate([p["pt_X"] for p in probs])
        t = time.perf_counter()
        batch = BaBatch(probs)
        t_create = (time.perf_counter() - t) * 1e3
        batch._owner.set_stream(stream.cuda_stream)
        res = []

        def run_batch():
            batch.update_values(T0, X0)
            res[:] = batch.solve(opt, cap=0)[1]
        ms_batch = timed(run_batch)
        assert all(r.status == 0 and r.n_iter == a.iters for r in res)
        info = batch.info()
        batch.close()

        t = time.perf_counter()
        hs = []
        for p in probs:
            h = BaProblem(0)
            h.set_cameras(p["cam_intr"], p["cam_T"])
            h.set_poses(p["pose_T"], p["pose_fixed"])
            h.set_points(p["pt_X"], p["pt_fixed"])
            h.set_observations(p["obs_cam"], p["obs_pose"], p["obs_pt"], p["obs_uv"])
            h.set_stream(stream.cuda_stream)
            h.finalize()
            hs.append(h)
        t_final = (time.perf_counter() - t) * 1e3

        def run_loop():
            for h, p in zip(hs, probs):
                h.update_values(p["pose_T"], p["pt_X"])
                h.solve(opt)
        ms_loop = timed(run_loop)
        for h in hs:
            h.close()
        lines.append("B = %4d  %d LM iterations  batch %9.3f ms   loop of handles %10.3f ms   "
                     "ratio x%.1f   (planning: ba_batch_create %.1f ms, %d x ba_finalize %.1f ms; "
                     "LDS %d B / workgroup, image %d columns)"
                     % (B, a.iters, ms_batch, ms_loop, ms_loop / ms_batch, t_create, B, t_final,
                        info["lds_bytes"], info["image_columns"]))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("full_batch_bench: windows of 10 poses / 300 landmarks, stereo, sigma 0.5 px; "
                     "device time by hipEvents, best of %d\n" % a.reps)
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
