"""Cost of relative-pose factors on the batch path (ba_batch_set_relative as more factors of
ba_batch_solve).  B windows of 10 poses / 300 landmarks, stereo, sigma = 0.5 px (the windows
of batch_prior_bench.py) with one pose fixed: 9 optimisable poses, a 64-column image.  10 LM
iterations with both thresholds at 0, so that every run does the same work.

  none         ba_batch_solve, no factors set;
  chain        the same with an odometry chain on every window: 9 factors (q + 1, q) over
               consecutive poses (the first ends on the fixed pose), Z = the relative pose of
               the start values moved by a 1e-2 tangent, Omega = J^T J of a seeded random J;
  chain+prior  the chain plus a K = 9 prior on every window (batch_prior_bench.synthetic_prior).

Device time by hipEvents on the stream the work runs on, best of --reps after one warm-up;
the values are reset before every solve (outside the timed span).

With --parent-lib the `none` figure is also taken --rounds times, in fresh processes that
alternate between that library (the parent commit's build) and this one: the factors must not
slow down a batch that has none, so the median of this library's figures must not exceed the
parent's slowest run, the upper end of its own run-to-run spread (the tool
says on its last lines which holds and exits with 1 if this library is slower).  The overhead
of the chain is reported, not gated.

    python tools/batch_relative_bench.py [--B 64 1000] [--parent-lib PATH] [--out profiles/batch_relative_v1.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_prior_bench import synthetic_prior, windows  # noqa: E402

ITERS = 10
NEW_SYMBOLS = ("ba_batch_set_relative", "ba_batch_relative_check", "ba_batch_relative_info",
               "ba_batch_relative_marg_plan")


def load_binding():
    """the package's binding; a library from before the factors (the parent commit's, named by
    BA_HIP_LIB) is driven through the same binding without the symbols it does not have"""
    from bundle_adjustment_solver_amd import _lib
    _lib.load(optional=NEW_SYMBOLS)
    return _lib.has_symbol("ba_batch_set_relative")


def odometry_chain(pr, seed):
    """9 factors (q + 1, q), q = 0 .. 8, on a window of 10 poses whose pose 0 is fixed"""
    rng = np.random.default_rng(seed)
    T = np.asarray(pr["pose_T"], np.float64)
    n = T.shape[0]
    j, k = np.arange(1, n, dtype=np.int32), np.arange(0, n - 1, dtype=np.int32)
    Z, Om = np.zeros((n - 1, 12)), np.zeros((n - 1, 6, 6))
    for f in range(n - 1):
        Rj, tj = T[j[f], :9].reshape(3, 3), T[j[f], 9:]
        Rk, tk = T[k[f], :9].reshape(3, 3), T[k[f], 9:]
        R = Rj @ Rk.T
        Z[f, :9] = R.reshape(9)
        Z[f, 9:] = tj - R @ tk + 1e-2 * rng.standard_normal(3) / np.sqrt(3.0)
        J = rng.standard_normal((8, 6)) * 30.0
        Om[f] = J.T @ J
    return dict(j=j, k=k, Z=Z, Omega=Om)


def measure(Bs, reps, distinct, with_factors):
    """-> {B: {"none": ms, "chain": ms, "chain+prior": ms}} (the last two only if asked)"""
    has_rel = load_binding()
    import torch
    from bundle_adjustment_solver_amd._lib import make_options
    from bundle_adjustment_solver_amd.solver import BaBatch
    stream = torch.cuda.Stream()
    base = windows(distinct)
    opt = make_options(max_iter=ITERS, thr_step=0.0, thr_cost=0.0)
    out = {}

    def timed(fn, reset):
        best = float("inf")
        for r in range(reps + 1):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            if r > 0:
                best = min(best, e0.elapsed_time(e1))
        return best

    for B in Bs:
        probs = [base[k % len(base)] for k in range(B)]
        batch = BaBatch(probs)
        batch._owner.set_stream(stream.cuda_stream)
        T0, X0 = batch.get_poses(), batch.get_points()
        reset = lambda: batch.update_values(T0, X0)
        res = []

        def solve():
            res[:] = batch.solve(opt, cap=0)[1]
        row = {"none": timed(solve, reset)}
        assert all(r.status == 0 and r.n_iter == ITERS for r in res)
        if with_factors and has_rel:
            batch.set_relative([odometry_chain(base[k % len(base)], 200 + k % len(base)) for k in range(B)])
            row["chain"] = timed(solve, reset)
            assert all(r.status == 0 and r.n_iter == ITERS for r in res)
            batch.set_prior([synthetic_prior(base[k % len(base)], 100 + k % len(base)) for k in range(B)])
            row["chain+prior"] = timed(solve, reset)
            assert all(r.status == 0 and r.n_iter == ITERS for r in res)
            row["image_columns"] = batch.info()["image_columns"]
            row["factor_bytes"] = batch.relative_info()["device_bytes"]
        batch.close()
        out[B] = row
    return out


def child(lib, Bs, reps, distinct, with_factors):
    env = dict(os.environ)
    if lib:
        env["BA_HIP_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps), "--distinct", str(distinct),
           "--B"] + [str(b) for b in Bs] + (["--with-factors"] if with_factors else [])
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("child failed:\n" + r.stdout)
    return {int(k): v for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[64, 1000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=16,
                    help="distinct windows generated; the batch cycles through them")
    ap.add_argument("--parent-lib", default=None, help="libba_hip.so built from the parent commit")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--with-factors", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.B, a.reps, a.distinct, a.with_factors)))
        return 0
    lines = []
    got = child(None, a.B, a.reps, a.distinct, True)
    for B in a.B:
        r = got[B]
        lines.append("B = %4d  %d iterations  no factors %9.3f ms   odometry chain of 9 factors per window %9.3f ms "
                     "(+%.1f %%)   chain plus a K = 9 prior %9.3f ms (+%.1f %%)   "
                     "(image %d columns, %d bytes of factor records and scratch)"
                     % (B, ITERS, r["none"], r["chain"], 100.0 * (r["chain"] / r["none"] - 1.0), r["chain+prior"],
                        100.0 * (r["chain+prior"] / r["none"] - 1.0), r["image_columns"], r["factor_bytes"]))
        print(lines[-1], flush=True)
    ok = True
    if a.parent_lib:
        par, new = [], []
        for _ in range(a.rounds):           # alternate, fresh processes
            par.append(child(os.path.abspath(a.parent_lib), a.B, a.reps, a.distinct, False))
            new.append(child(None, a.B, a.reps, a.distinct, False))
        for B in a.B:
            p = [x[B]["none"] for x in par]
            n = [x[B]["none"] for x in new]
            med = float(np.median(n))
            inside = med <= max(p)   # faster than the parent is no failure
            ok = ok and inside
            verdict = ("SLOWER than every run of the parent" if not inside else
                       "within the parent's spread" if med >= min(p) else
                       "not slower than the parent's runs (median below the parent's fastest)")
            lines.append("B = %4d  no factors, %d fresh processes each, alternating: parent commit %s ms "
                         "(spread %.3f .. %.3f)   this commit %s ms   %s"
                         % (B, a.rounds, " ".join("%.3f" % v for v in p), min(p), max(p),
                            " ".join("%.3f" % v for v in n), verdict))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("batch_relative_bench: windows of 10 poses (1 fixed) / 300 landmarks, stereo, sigma 0.5 px, %d LM "
                     "iterations; device time by hipEvents, best of %d\n" % (ITERS, a.reps))
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
