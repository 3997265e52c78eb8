"""Throughput of the gradient-descent loop (ba_gd_*) at the BASELINE configs:
iterations enqueued in batches without host synchronisation (ba_gd_iterate),
timed over whole batches, beside the bytes one iteration moves (estimate from
the list sizes) and the implied bandwidth.  Usage: tools/gd_bench.py [C2 C3 C4 C4R]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bundle_adjustment_solver_amd import scenes  # noqa: E402
from bundle_adjustment_solver_amd._lib import make_options  # noqa: E402
from bundle_adjustment_solver_amd.solver import BaProblem  # noqa: E402

BATCH, REPS = 50, 5


def bytes_per_iteration(pr):
    """Reads and writes of one iteration, assuming every gather misses the caches:
    landmark-major pass (16 B record + 16 B uv + 24 B point + 96 B pose per
    observation), pose-major pass (8 B record + 16 B uv + 24 B point), update."""
    n_obs = len(pr["obs_uv"])
    free_pose = pr["pose_fixed"][pr["obs_pose"]] == 0
    n_pobs = int(free_pose.sum())
    N, M = int((pr["pose_fixed"] == 0).sum()), int((pr["pt_fixed"] == 0).sum())
    lm = n_obs * (16 + 16 + 24) + M * 24
    pm = n_pobs * (8 + 16 + 24)
    upd = N * (48 + 2 * 96) + M * (24 + 2 * 24)
    # the same without the point gathers of the landmark-major pass (consecutive
    # landmarks: each point is read once) and with the poses cached
    lean = n_obs * 32 + M * 24 + pm + upd
    return lm + pm + upd, lean


names = sys.argv[1:] or ["C2", "C3", "C4", "C4R"]
for name in names:
    sc = scenes.config_scene(name)
    pr = scenes.scaled_problem(sc)
    p = BaProblem(0)
    p.set_cameras(pr["cam_intr"], pr["cam_T"])
    p.set_poses(pr["pose_T"], pr["pose_fixed"])
    p.set_points(pr["pt_X"], pr["pt_fixed"])
    p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
    p.finalize()
    opt = make_options(max_iter=BATCH * (REPS + 1), thr_step=0.0, thr_cost=0.0)
    p.gd_begin(opt)
    p.gd_iterate(BATCH)          # warm-up batch
    p.gd_sync()
    ts = []
    for _ in range(REPS):
        t = time.perf_counter()
        p.gd_iterate(BATCH)
        p.gd_sync()
        ts.append((time.perf_counter() - t) / BATCH)
    rows, n_it, _, _ = p.gd_sync(cap=BATCH * (REPS + 1))
    assert n_it == BATCH * (REPS + 1)
    worst, lean = bytes_per_iteration(pr)
    ms = min(ts) * 1e3
    print("%-4s obs %9d  GD iteration %.4f ms (median %.4f)  %7.0f it/s  "
          "bytes/it %.3f GB (all gathers missing) %.3f GB (lean) -> %.2f / %.2f TB/s  "
          "cost %.6e -> %.6e" % (name, len(pr["obs_uv"]), ms, sorted(ts)[len(ts) // 2] * 1e3,
                                 1e3 / ms, worst / 1e9, lean / 1e9, worst / ms / 1e9,
                                 lean / ms / 1e9, rows[0].cost, rows[-1].cost), flush=True)
    p.close()
