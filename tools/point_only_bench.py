"""Point-only solve (ba_point_only: every pose fixed, a team of lanes per landmark, one
launch) at the C4 size: 1 000 poses, 500 k landmarks, 5 M stereo observations (10 per
landmark), points at the scene's perturbed start values.

Reported, per team width (8 and 16 lanes):
  * 10 LM iterations with both thresholds 0 — device time of the launch (hipEvents around
    it, ba_point_only_last_ms), best of 5 after one warm-up, and the host time of the
    whole call (packing, upload, launch, download);
  * the same with triangulation only (max_num_iterations = 0, every flag set).
Beside them:
  * the CPU oracle on a sample of 1 000 one-landmark problems, SCALED to all landmarks
    (single thread; it is what a caller had before);
  * k_lin_grp's time for one pass over the same observations (the handle path's
    linearisation of the same scene, per-kernel event timing): the yardstick for what
    one linearisation pass costs on this part.

    python tools/point_only_bench.py [--scale 1.0] [--out profiles/point_only_v1.txt]
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
from bundle_adjustment_solver_amd.solver import (BaProblem, point_only, point_only_last_ms,  # noqa: E402
                                                 point_only_team)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the C4 size")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pr = scenes.scaled_problem(scenes.config_scene("C4", scale=a.scale, pixel_sigma=0.5))
    n_pt, n_obs = pr["pt_X"].shape[0], pr["obs_pt"].size
    lines = ["point_only_bench: %d poses, %d landmarks, %d observations (stereo, sigma 0.5 px); "
             "device time by hipEvents around the launch, best of %d"
             % (pr["pose_T"].shape[0], n_pt, n_obs, a.reps)]
    print(lines[0], flush=True)
    h = BaProblem(0)
    opt = make_options(max_iter=a.iters, thr_step=0.0, thr_cost=0.0)
    opt0 = make_options(max_iter=0)
    args = (pr["cam_intr"], pr["cam_T"], pr["pose_T"], pr["pt_X"], pr["obs_cam"], pr["obs_pose"],
            pr["obs_pt"], pr["obs_uv"])
    default = point_only_team(0)

    def timed(o, tri):
        best_dev, best_host, out = float("inf"), float("inf"), None
        for r in range(a.reps + 1):
            t = time.perf_counter()
            out = point_only(h, *args, o, triangulate=tri, cap=0)
            host = (time.perf_counter() - t) * 1e3
            if r > 0:
                best_dev, best_host = min(best_dev, point_only_last_ms()), min(best_host, host)
        return best_dev, best_host, out

    for w in (8, 16):
        point_only_team(w)
        dev, host, (X, res, _) = timed(opt, None)
        assert (res.status == 0).all() and (res.n_iter == a.iters).all()
        lines.append("team %2d  %d LM iterations      launch %9.3f ms   whole call %9.1f ms   "
                     "(%.1f ps per observation and iteration; cost %.6e -> %.6e)"
                     % (w, a.iters, dev, host, dev * 1e9 / (n_obs * a.iters), res.cost0.sum(), res.cost.sum()))
        print(lines[-1], flush=True)
        dev, host, (X, res, _) = timed(opt0, np.ones(n_pt, np.uint8))
        assert (res.status == 0).all()
        lines.append("team %2d  triangulation only     launch %9.3f ms   whole call %9.1f ms   "
                     "(%d landmarks with an observation behind its camera)"
                     % (w, dev, host, int((res.n_behind > 0).sum())))
        print(lines[-1], flush=True)
    point_only_team(default)
    lines.append("default team width of the library: %d" % default)

    # the CPU oracle on a sample of one-landmark problems, scaled
    from oracle import oracle_py as O
    order = np.argsort(pr["obs_pt"], kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(pr["obs_pt"], minlength=n_pt))])
    sample = np.linspace(0, n_pt - 1, min(a.sample, n_pt)).astype(int)
    t = time.perf_counter()
    for i in sample:
        idx = order[off[i]:off[i + 1]]
        o = O.Oracle(dict(cam_intr=pr["cam_intr"], cam_T=pr["cam_T"], pose_T=pr["pose_T"],
                          pose_fixed=np.ones(pr["pose_T"].shape[0], np.uint8), pt_X=pr["pt_X"][[i]],
                          pt_fixed=np.zeros(1, np.uint8), obs_cam=pr["obs_cam"][idx],
                          obs_pose=pr["obs_pose"][idx], obs_pt=np.zeros(idx.size, np.int32),
                          obs_uv=pr["obs_uv"][idx]))
        o.solve(O.make_options(max_iter=a.iters, thr_step=0.0, thr_cost=0.0))
        o.close()
    cpu = (time.perf_counter() - t) * 1e3
    lines.append("CPU oracle, %d LM iterations: %.1f ms for %d one-landmark problems (problem set-up "
                 "included), SCALED to %d landmarks: %.0f ms" % (a.iters, cpu, sample.size, n_pt,
                                                                  cpu * n_pt / sample.size))
    print(lines[-1], flush=True)

    # k_lin_grp: one linearisation pass of the handle path over the same observations
    p = BaProblem(0)
    p.set_cameras(pr["cam_intr"], pr["cam_T"])
    p.set_poses(pr["pose_T"], pr["pose_fixed"])
    p.set_points(pr["pt_X"], pr["pt_fixed"])
    p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
    p.finalize()
    p.solve(make_options(max_iter=2, thr_step=0.0, thr_cost=0.0))       # warm-up
    p.enable_stage_timing(True)
    p.get_kernel_ms(reset=True)
    p.solve(make_options(max_iter=5, thr_step=0.0, thr_cost=0.0))
    km = p.get_kernel_ms()
    for name in ("k_lin_grp", "k_lin_landmarks"):
        if name in km and km[name][1] > 0:
            lines.append("handle path, %s: %.1f us per launch (%d launches; one linearisation pass "
                         "of the full problem's landmark side)" % (name, km[name][0] * 1e3 / km[name][1],
                                                                    km[name][1]))
            print(lines[-1], flush=True)
    p.close()
    h.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
