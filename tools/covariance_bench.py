"""ba_covariance at config C4 (N = 995 optimisable poses) against the route a caller had
before it: get_S() (download of the dense reduced system) + numpy.linalg.inv on the host.

Timed with events on the handle's stream around the whole call (linearisation at
lambda = 0, Schur complement, factorisation, the covariance kernels, the result copies),
best of 5 after one warm-up.  The call synchronises the stream a few times on the way, so
the figure is the stream's elapsed time, not the sum of kernel times.  The host route is
wall time (download + inverse), measured once.

    python tools/covariance_bench.py [--config C4] [--scale 1.0] [--points 10000] [--out profiles/covariance_v1.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bundle_adjustment_solver_amd import scenes  # noqa: E402
from bundle_adjustment_solver_amd.solver import BaProblem  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C4")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the get_S + numpy.linalg.inv route")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    stream = torch.cuda.Stream()
    pr = scenes.scaled_problem(scenes.config_scene(a.config, scale=a.scale))
    p = BaProblem(0)
    p.set_cameras(pr["cam_intr"], pr["cam_T"])
    p.set_poses(pr["pose_T"], pr["pose_fixed"])
    p.set_points(pr["pt_X"], pr["pt_fixed"])
    p.set_observations(pr["obs_cam"], pr["obs_pose"], pr["obs_pt"], pr["obs_uv"])
    p.set_stream(stream.cuda_stream)
    p.finalize()
    ps = np.nonzero(pr["pose_fixed"] == 0)[0]
    qs = np.nonzero(pr["pt_fixed"] == 0)[0]
    qs = qs[np.linspace(0, qs.size - 1, min(a.points, qs.size)).astype(np.int64)]
    dense = p.get_dense_info()
    lines = ["config %s scale %g: N %d optimisable poses, npad %d, tile fill %.3f, %d levels"
             % (a.config, a.scale, p.N, dense["npad"], dense["fill"], dense["levels"])]

    def timed(pose_sel, pt_sel):
        best, out = None, None
        for rep in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = p.covariance(pose_sel, pt_sel, 1.0)
            e1.record(stream)
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if rep > 0:
                best = ms if best is None else min(best, ms)
        return best, out

    ms_p, (cp, _, dropped) = timed(ps, [])
    info = p.covariance_info()
    lines.append("all %d pose blocks: %.3f ms (best of %d), %d batch(es) of %d columns, dropped pivots %d"
                 % (ps.size, ms_p, a.reps, info["last_batches"], info["batch_cols"], dropped))
    ms_pq, (_, cq, dropped) = timed(ps, qs)
    info = p.covariance_info()
    lines.append("all %d pose blocks + %d landmark blocks: %.3f ms (best of %d), %d batch(es), dropped pivots %d"
                 % (ps.size, qs.size, ms_pq, a.reps, info["last_batches"], dropped))
    # only the factorisation part, for the split: an empty selection runs everything but the sweeps
    ms_0, _ = timed([], [])
    lines.append("empty selection (linearise + Schur + factorise only): %.3f ms" % ms_0)
    # MFMA work of the pose sweep, an UPPER bound from the schedule's fill (a wave visits at most every
    # non-zero tile: nb/4 * nb/16 instructions per off-diagonal tile, 4 np (np - 1) / 2 + 8 np per diagonal
    # tile, np = nb / 16; the rows above a column's first non-zero are skipped, so it executes fewer)
    npad = dense["npad"]
    nb = 32 if npad == 32 * ((p.N + 4) // 5) else 64   # (5 poses per 32-column tile, 10 per 64-column tile)
    ncb, npn = npad // nb, nb // 16
    nnz_off = max(0.0, dense["fill"] * ncb * (ncb + 1) / 2 - ncb)
    waves = (ps.size + 1) // 2
    mfma = waves * (nnz_off * (nb // 4) * npn + ncb * (2 * npn * (npn - 1) + 8 * npn))
    lines.append("pose sweep: <= %.3e v_mfma_f64_16x16x4 (%d waves, tile order %d, %.0f non-zero off-diagonal tiles) "
                 "= <= %.3e flop in %.3f ms (all-pose call minus empty call): <= %.2f TFLOP/s"
                 % (mfma, waves, nb, nnz_off, mfma * 2048, ms_p - ms_0, mfma * 2048 / ((ms_p - ms_0) * 1e-3) / 1e12))
    if not a.no_host:
        t0 = time.perf_counter()
        S, _ = p.get_S()
        t1 = time.perf_counter()
        Si = np.linalg.inv(S)
        t2 = time.perf_counter()
        hp = np.stack([Si[6 * j:6 * j + 6, 6 * j:6 * j + 6] for j in range(p.N)])
        err = max(np.abs(x - y).max() / np.abs(y).max() for x, y in zip(cp, hp))
        lines.append("host route: get_S %.1f ms (%.0f MB) + numpy.linalg.inv %.1f ms = %.1f ms; "
                     "pose blocks agree to %.2e relative; no landmark blocks on this route"
                     % ((t1 - t0) * 1e3, S.nbytes / 1e6, (t2 - t1) * 1e3, (t2 - t0) * 1e3, err))
    p.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
