"""Throughput of the batched planar 3-DoF pose-only solvers
(ba_pose_only_{mono,stereo}3_batch: one workgroup per problem, one launch per
batch) against the same frames solved by a loop of single calls
(ba_pose_only_{mono,stereo}3: one pack + H2D + launch + D2H + sync each), for B
in {64, 1000} problems of n in {200, 500, 2000} points.  Per case: the median of
the batched host call, of the loop, of the device-tensor path (torch events
around the enqueue on the current stream; inputs and planar records already on
the GPU), and the per-frame microseconds.

  python tools/planar_batch_bench.py [--reps R]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bundle_adjustment_solver_amd import scenes  # noqa: E402
from bundle_adjustment_solver_amd._lib import make_options  # noqa: E402
from bundle_adjustment_solver_amd.solver import BaProblem  # noqa: E402
from pose_only_batch_bench import KW, median_ms, to12  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    g = BaProblem(0)
    opt = make_options(**KW)
    dev = torch.device("cuda", 0)
    for stereo in (False, True):
        for B in (64, 1000):
            for n in (200, 500, 2000):
                sc = scenes.planar_pose_only_batch_scene(B, n, n, seed=2026, stereo=stereo,
                                                         pixel_sigma=0.5,
                                                         right_missing_frac=0.2,
                                                         outlier_frac=0.05)
                o, N = sc["offsets"], sc["offsets"][-1]
                P = {k: np.stack([to12(t) for t in sc[k]])
                     for k in ("T_bc", "T_wl", "T_wc_init") + (("T_lr",) if stereo else ())}
                T = P["T_wc_init"]
                ones = np.ones(N, np.uint8)
                if stereo:
                    batch = lambda: g.pose_only_stereo3_batch(
                        o, sc["X"], sc["uv"], sc["uv_right"], sc["intr"], sc["intr_r"],
                        P["T_bc"], P["T_lr"], P["T_wl"], T, ones, ones, opt)

                    def loop():
                        for b in range(B):
                            s = slice(o[b], o[b + 1])
                            g.pose_only_stereo3(sc["X"][s], sc["uv"][s], sc["uv_right"][s],
                                                sc["intr"][b], sc["intr_r"][b], P["T_bc"][b],
                                                P["T_lr"][b], P["T_wl"][b], T[b], ones[s],
                                                ones[s], opt)
                else:
                    batch = lambda: g.pose_only_mono3_batch(o, sc["X"], sc["uv"], sc["intr"],
                                                            P["T_bc"], P["T_wl"], T, ones, opt)

                    def loop():
                        for b in range(B):
                            s = slice(o[b], o[b + 1])
                            K = [float(v) for v in sc["intr"][b]]
                            g.pose_only_mono3(sc["X"][s], sc["uv"][s], *K, P["T_bc"][b],
                                              P["T_wl"][b], T[b], ones[s], opt)
                res = batch()
                iters = np.mean([r["n_iter"] for r in res])
                t_batch = median_ms(batch, args.reps)
                t_loop = median_ms(loop, max(1, args.reps // 3))
                d = lambda a, t=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=t,
                                                               device=dev)
                rec = d(BaProblem.planar_records(P["T_bc"], P["T_wl"], T,
                                                 P["T_lr"] if stereo else None,
                                                 sc["intr_r"] if stereo else None))
                targs = [d(o, torch.int32), d(sc["X"]), d(sc["uv"])]
                mt = d(ones, torch.uint8)
                if stereo:
                    targs += [d(sc["uv_right"]), d(sc["intr"]), rec, d(T), mt, mt.clone()]
                    call = lambda: g.pose_only_stereo3_batch_tensors(*targs, opt)
                else:
                    targs += [d(sc["intr"]), rec, d(T), mt]
                    call = lambda: g.pose_only_mono3_batch_tensors(*targs, opt)
                call()
                torch.cuda.synchronize()
                ev = []
                for _ in range(args.reps):
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call()
                    e1.record()
                    ev.append((e0, e1))
                torch.cuda.synchronize()
                t_dev = float(np.median([a.elapsed_time(b) for a, b in ev]))
                print("%s B=%4d n=%4d  GN iters %.1f  batch %.3f ms  loop %.2f ms  "
                      "(x%.1f)  device-tensor %.3f ms  per frame: batch %.2f us, loop %.1f us, "
                      "device %.2f us" %
                      ("stereo" if stereo else "mono  ", B, n, iters, t_batch, t_loop,
                       t_loop / t_batch, t_dev, t_batch * 1e3 / B, t_loop * 1e3 / B,
                       t_dev * 1e3 / B), flush=True)


if __name__ == "__main__":
    main()
