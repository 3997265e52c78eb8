"""Batched marginalisation priors (ba_batch_marginalize, one workgroup per window, one
launch) against what a caller could do before it: per window a finalized handle over the
sub-problem of the landmarks in L (every observation of a landmark the marked pose sees),
ba_stage_linearize(0, huber), ba_stage_schur and ba_get_S, then the elimination of the
marked pose's six columns in numpy on the host.  B windows of 10 poses / ~300 landmarks,
stereo, sigma = 0.5 px (the windows of full_batch_bench.py), Huber threshold 1.0, the oldest
optimisable pose marked.

Both sides are timed with hipEvents on the stream the work runs on, best of 5 after one
warm-up (the loop's figure therefore contains its host work between the launches: the copy
of S and the numpy elimination, which are part of that route); planning (ba_batch_create /
ba_finalize) is excluded from both and reported separately.

    python tools/batch_marginalize_bench.py [--B 64 1000] [--out profiles/batch_marginalize_v1.txt]
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


def host_prior(S, rhs, m6):
    """eliminate the first m6 columns of the reduced camera system (marked pose first)"""
    S = np.tril(S) + np.tril(S, -1).T
    Smm, Skm = S[:m6, :m6], S[m6:, :m6]
    sol = np.linalg.solve(Smm, np.column_stack([Skm.T, rhs[:m6]]))
    return S[m6:, m6:] - Skm @ sol[:, :-1], rhs[m6:] - Skm @ sol[:, -1]


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
        marks = []
        for p in probs:
            mk = np.zeros(len(p["pose_fixed"]), np.uint8)
            mk[np.flatnonzero(p["pose_fixed"] == 0)[0]] = 1   # the oldest optimisable pose
            marks.append(mk)
        mark = np.concatenate(marks)
        t = time.perf_counter()
        batch = BaBatch(probs)
        t_create = (time.perf_counter() - t) * 1e3
        batch._owner.set_stream(stream.cuda_stream)
        got = []

        def run_batch():
            got[:] = batch.marginalize(mark, a.huber)
        ms_batch = timed(run_batch)
        assert all(r.status == 0 and r.dropped_pivots == 0 for r in got[3])
        n_l = sum(r.n_marg_pt for r in got[3])

        t = time.perf_counter()
        hs = []
        for p, mk in zip(probs, marks):
            in_l = np.zeros(len(p["pt_fixed"]), bool)
            in_l[p["obs_pt"][mk[p["obs_pose"]] != 0]] = True
            keep = (in_l & (p["pt_fixed"] == 0))[p["obs_pt"]]
            # the marked pose is the oldest optimisable one: it owns the first six columns of S
            h = BaProblem(0)
            h.set_cameras(p["cam_intr"], p["cam_T"])
            h.set_poses(p["pose_T"], p["pose_fixed"])
            h.set_points(p["pt_X"], p["pt_fixed"])
            h.set_observations(p["obs_cam"][keep], p["obs_pose"][keep], p["obs_pt"][keep], p["obs_uv"][keep])
            h.set_stream(stream.cuda_stream)
            h.finalize()
            hs.append(h)
        t_final = (time.perf_counter() - t) * 1e3
        loop = []

        def run_loop():
            loop.clear()
            for h in hs:
                h.stage_linearize(0.0, a.huber)
                h.stage_schur()
                loop.append(host_prior(*h.get_S(), 6))
        ms_loop = timed(run_loop)
        for h in hs:
            h.close()
        # the two routes describe the same prior
        worst = 0.0
        for p in range(min(B, a.distinct)):
            for x, y in ((got[0][p], loop[p][0]), (got[1][p], loop[p][1])):
                worst = max(worst, float(np.abs(x - y).max() / np.abs(y).max()))
        K = got[3][0].n_kept
        batch.close()
        lines.append("B = %4d  %d kept poses per window, %d landmarks marginalised  batch %9.3f ms   "
                     "loop of handles + numpy %10.3f ms   ratio x%.1f   largest relative difference between the "
                     "routes %.1e   (planning: ba_batch_create %.1f ms, %d x ba_finalize %.1f ms; image %d columns)"
                     % (B, K, n_l, ms_batch, ms_loop, ms_loop / ms_batch, worst, t_create, B, t_final,
                        16 * -(-(16 + 6 * K) // 16)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("batch_marginalize_bench: windows of 10 poses / 300 landmarks, stereo, sigma 0.5 px, the oldest "
                     "optimisable pose marked; device time by hipEvents, best of %d\n" % a.reps)
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
