"""Batched covariance (ba_batch_covariance, one workgroup per window, one launch) against
the route that existed before it: a loop of finalized handles, each calling ba_covariance
for all of its free poses and points.  B windows of 10 poses / ~300 landmarks, stereo,
sigma = 0.5 px (the windows of full_batch_bench.py), Huber threshold 1.0, every landmark
block asked for on both sides.

Both sides are timed with hipEvents on the stream the work runs on, best of 5 after one
warm-up; planning (ba_batch_create / ba_finalize) is excluded from both and reported
separately.

    python tools/batch_covariance_bench.py [--B 64 1000] [--out profiles/batch_covariance_v1.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bundle_adjustment_solver_amd import scenes  # noqa: E402
from bundle_adjustment_solver_amd.solver import BaBatch, BaProblem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 1000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--huber", type=float, default=1.0)
    ap.add_argument("--distinct", type=int, default=16,
                    help="distinct windows generated; the batch cycles through them")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
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
        t = time.perf_counter()
        batch = BaBatch(probs)
        t_create = (time.perf_counter() - t) * 1e3
        batch._owner.set_stream(stream.cuda_stream)
        got = []

        def run_batch():
            got[:] = batch.covariance(a.huber, points=True)
        ms_batch = timed(run_batch)
        assert all(r.status == 0 and r.dropped_pivots == 0 for r in got[2])
        info = batch.info()

        t = time.perf_counter()
        hs, sel = [], []
        for p in probs:
            h = BaProblem(0)
            h.set_cameras(p["cam_intr"], p["cam_T"])
            h.set_poses(p["pose_T"], p["pose_fixed"])
            h.set_points(p["pt_X"], p["pt_fixed"])
            h.set_observations(p["obs_cam"], p["obs_pose"], p["obs_pt"], p["obs_uv"])
            h.set_stream(stream.cuda_stream)
            h.finalize()
            hs.append(h)
            sel.append((np.nonzero(p["pose_fixed"] == 0)[0], np.nonzero(p["pt_fixed"] == 0)[0]))
        t_final = (time.perf_counter() - t) * 1e3
        loop = []

        def run_loop():
            loop[:] = [h.covariance(ps, qs, a.huber) for h, (ps, qs) in zip(hs, sel)]
        ms_loop = timed(run_loop)
        for h in hs:
            h.close()
        # the two routes describe the same blocks
        worst = 0.0
        for p in range(min(B, a.distinct)):
            ps, qs = sel[p]
            for x, y in ((batch.cov_poses_of(p, got[0])[ps], loop[p][0]),
                         (batch.cov_points_of(p, got[1])[qs], loop[p][1])):
                scale = np.abs(y).reshape(len(y), -1).max(axis=1)
                worst = max(worst, float((np.abs(x - y).reshape(len(y), -1).max(axis=1) / scale).max()))
        batch.close()
        n_blk = sum(len(ps) for ps, _ in sel), sum(len(qs) for _, qs in sel)
        lines.append("B = %4d  %d pose + %d landmark blocks  batch %9.3f ms   loop of handles %10.3f ms   "
                     "ratio x%.1f   largest relative block difference between the routes %.1e   "
                     "(planning: ba_batch_create %.1f ms, %d x ba_finalize %.1f ms; image %d columns)"
                     % (B, n_blk[0], n_blk[1], ms_batch, ms_loop, ms_loop / ms_batch, worst, t_create, B,
                        t_final, info["image_columns"]))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("batch_covariance_bench: windows of 10 poses / 300 landmarks, stereo, sigma 0.5 px, all pose "
                     "and landmark blocks; device time by hipEvents, best of %d\n" % a.reps)
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
