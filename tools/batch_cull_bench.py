"""The two-stage local BA of the batch path (ba_batch_solve_culled: solve, cull, solve in one
go) against its two solves alone and against the host route a caller had before: B windows
of 10 poses / 300 landmarks, stereo, sigma = 0.3 px, 5 % of the observations displaced by
30..80 px; 5 + 10 LM iterations (thresholds 0, Huber 2 px, lambda0 1e-3), cull at 25 px^2.

solve_culled and the two solves are timed with hipEvents on the stream the work runs on,
best of 5 after one warm-up; their difference is the price of the cull and the compaction.
The host route (solve, download, numpy re-projection, a new ba_batch_create without the
outliers, solve) is wall time, best of 3: it has host work between its launches.

    python tools/batch_cull_bench.py [--B 64 1000] [--out profiles/batch_cull_v1.txt]
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
from bundle_adjustment_solver_amd.solver import BaBatch  # noqa: E402

OBS_KEYS = ("obs_cam", "obs_pose", "obs_pt", "obs_uv")
E2_MAX = 25e-4


def displaced(sc, seed):
    rng = np.random.default_rng(seed)
    n = sc["obs_pt"].size
    idx = rng.choice(n, n // 20, replace=False)
    ang, mag = rng.uniform(0, 2 * np.pi, idx.size), rng.uniform(30.0, 80.0, idx.size)
    sc["obs_uv"] = sc["obs_uv"].copy()
    sc["obs_uv"][idx] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
    return sc


def project(pr, T, X):
    oc, op, oq = pr["obs_cam"], pr["obs_pose"], pr["obs_pt"]
    P, Cm, intr = T[op], pr["cam_T"][oc], pr["cam_intr"][oc]
    Xij = np.einsum("nij,nj->ni", P[:, :9].reshape(-1, 3, 3), X[oq]) + P[:, 9:]
    Xc = np.einsum("nij,nj->ni", Cm[:, :9].reshape(-1, 3, 3), Xij) + Cm[:, 9:]
    r0 = intr[:, 0] * (Xc[:, 0] / Xc[:, 2]) + intr[:, 2] - pr["obs_uv"][:, 0]
    r1 = intr[:, 1] * (Xc[:, 1] / Xc[:, 2]) + intr[:, 3] - pr["obs_uv"][:, 1]
    return r0 * r0 + r1 * r1, Xc[:, 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 1000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
    kw = dict(thr_step=0.0, thr_cost=0.0, huber=0.02, lambda0=1e-3)
    first, second = make_options(max_iter=5, **kw), make_options(max_iter=10, **kw)
    base = [scenes.scaled_problem(displaced(s, 100 + k)) for k, s in enumerate(
        scenes.ba_batch_scene(a.distinct, n_pose=10, n_pt=300, stereo=True, pixel_sigma=0.3))]
    lines = []

    def timed(fn, reps):
        best = float("inf")
        for r in range(reps + 1):
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
        batch = BaBatch(probs)
        batch._owner.set_stream(stream.cuda_stream)
        out = {}

        def run_culled():
            batch.set_obs_mask(None)
            batch.update_values(T0, X0)
            out["cres"] = batch.solve_culled(first, second, E2_MAX)[4]
        ms_culled = timed(run_culled, a.reps)
        n_culled = sum(c.n_culled for c in out["cres"])
        assert all(c.status == 0 and c.starved == 0 for c in out["cres"])

        def run_two():
            batch.set_obs_mask(None)
            batch.update_values(T0, X0)
            batch.solve(first, cap=0)
            batch.solve(second, cap=0)
        ms_two = timed(run_two, a.reps)

        def run_host():
            batch.set_obs_mask(None)
            batch.update_values(T0, X0)
            batch.solve(first, cap=0)
            T, X = batch.get_poses(), batch.get_points()
            kept = []
            for p, pr in enumerate(probs):
                e2, depth = project(pr, batch.poses_of(p, T), batch.points_of(p, X))
                on = (e2 <= E2_MAX) & (depth > 0)
                q = dict(pr, pose_T=batch.poses_of(p, T), pt_X=batch.points_of(p, X))
                for k in OBS_KEYS:
                    q[k] = pr[k][on]
                kept.append(q)
            nb = BaBatch(kept)
            nb._owner.set_stream(stream.cuda_stream)
            nb.solve(second, cap=0)
            nb.close()
        wall = float("inf")
        for r in range(4):
            t = time.perf_counter()
            run_host()
            if r > 0:
                wall = min(wall, (time.perf_counter() - t) * 1e3)
        batch.close()
        lines.append("B = %4d  5 + 10 LM iterations  solve_culled %9.3f ms   the two solves alone %9.3f ms   "
                     "cull + compaction %7.3f ms   host route (wall) %10.3f ms   (%d of %d observations culled)"
                     % (B, ms_culled, ms_two, ms_culled - ms_two, wall, n_culled,
                        sum(len(p["obs_pt"]) for p in probs)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("batch_cull_bench: windows of 10 poses / 300 landmarks, stereo, sigma 0.3 px, 5 %% displaced; "
                     "device time by hipEvents, best of %d; host route wall time, best of 3\n" % a.reps)
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
