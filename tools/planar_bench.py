"""Latency of the planar 3-DoF pose-only path (k_pose_only3): one
ba_pose_only_mono3 / ba_pose_only_stereo3 call = H2D copy + one persistent GN
kernel + D2H, vs the numpy restatement (tests/planar_pose_ref.py) on the same
inputs, at 10 k and 300 k points."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bundle_adjustment_solver_amd import scenes  # noqa: E402
from bundle_adjustment_solver_amd._lib import make_options  # noqa: E402
from bundle_adjustment_solver_amd.solver import BaProblem  # noqa: E402
import planar_pose_ref as R  # noqa: E402

KW = dict(max_iter=100, thr_step=1e-6, thr_cost=1e-6, huber=1.0, outlier=2.5)
to12 = lambda T: np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]).astype(np.float32)

g = BaProblem(0)
opt = make_options(**KW)
for stereo in (False, True):
    for n in (10_000, 300_000):
        sc = scenes.planar_pose_only_scene(n, seed=2026, pixel_sigma=0.5, stereo=stereo)
        ones = np.ones(n, np.uint8)
        intr = [sc["fx"], sc["fy"], sc["cx"], sc["cy"]]

        def call():
            if stereo:
                return g.pose_only_stereo3(sc["X"], sc["uv"], sc["uv_right"], intr, intr,
                                           to12(sc["T_bc"]), to12(sc["T_lr"]),
                                           to12(sc["T_wl"]), to12(sc["T_wc_init"]),
                                           ones, ones, opt)
            return g.pose_only_mono3(sc["X"], sc["uv"], *intr, to12(sc["T_bc"]),
                                     to12(sc["T_wl"]), to12(sc["T_wc_init"]), ones, opt)
        call()  # warm-up (module load, buffer growth)
        ts = []
        for r in range(15):
            t = time.perf_counter()
            res = call()
            ts.append(time.perf_counter() - t)
        kw = dict(KW)
        if stereo:
            kw.update(uv_right=sc["uv_right"], T_lr=sc["T_lr"], mask_r=ones.astype(bool),
                      intr_r=intr)
        t = time.perf_counter()
        ref = R.solve(sc["X"], sc["uv"], *intr, sc["T_bc"], sc["T_wl"], sc["T_wc_init"],
                      ones.astype(bool), **kw)
        tc = time.perf_counter() - t
        print("%s n=%d  iters gpu/cpu %d/%d  gpu call median %.3f ms (min %.3f)  "
              "cpu restatement (numpy) %.3f ms  max|dT| %.2e" %
              ("stereo" if stereo else "mono  ", n, res["n_iter"], ref["n_iter"],
               np.median(ts) * 1e3, min(ts) * 1e3, tc * 1e3,
               np.abs(res["T12"] - ref["T12"]).max()))
