"""Cost of a pose prior on the batch path (ba_batch_set_prior as one more factor of
ba_batch_solve).  B windows of 10 poses / 300 landmarks, stereo, sigma = 0.5 px (the windows
of full_batch_bench.py) with one pose fixed: 9 optimisable poses, a 64-column image.  10 LM
iterations with both thresholds at 0, so that every run does the same work.

  without    ba_batch_solve, no prior set;
  with       the same with a K = 9 prior on every window (H = J^T J of a seeded random J with
             51 rows: singular; T_lin = the start values moved by a 1e-2 tangent);
  slide      solve, ba_batch_marginalize of the oldest optimisable pose, ba_batch_set_prior of
             the result on the 8 kept poses (T_lin = the held values), solve again: what one
             step of a fixed-lag smoother costs on a batch whose next windows have this size.

Device time by hipEvents on the stream the work runs on, best of --reps after one warm-up;
the values are reset before every solve (outside the timed span).

With --parent-lib the `without` figure is also taken --rounds times, in fresh processes
that alternate between that library (the parent commit's build) and this one: the prior must
not slow down a batch that has none, so the median of this library's figures must not exceed
the parent's slowest run, the upper end of its own run-to-run spread (the tool says on its
last lines which holds, also when this library is faster than every run of the parent, and
exits with 1 if it is slower).

    python tools/batch_prior_bench.py [--B 64 1000] [--parent-lib PATH] [--out profiles/batch_prior_v1.txt]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ITERS = 10


def load_binding():
    """the package's binding; a library from before the prior (the parent commit's, named by
    BA_HIP_LIB) is driven through the same binding without the symbols it does not have"""
    from bundle_adjustment_solver_amd import _lib
    _lib.load(optional=("ba_batch_set_prior", "ba_batch_prior_check", "ba_batch_prior_info"))
    return _lib.has_symbol("ba_batch_set_prior")


def windows(distinct):
    from bundle_adjustment_solver_amd import scenes
    return [scenes.scaled_problem(s) for s in
            scenes.ba_batch_scene(distinct, n_pose=10, n_pt=300, stereo=True, pixel_sigma=0.5, n_fixed=1)]


def synthetic_prior(pr, seed):
    """K = 9: every optimisable pose; the size of H follows the window's own pose blocks"""
    rng = np.random.default_rng(seed)
    poses = np.flatnonzero(pr["pose_fixed"] == 0).astype(np.int32)
    n = 6 * len(poses)
    J = rng.standard_normal((n - 3, n)) * 30.0
    T = np.asarray(pr["pose_T"], np.float64)[poses].copy()
    T[:, 9:] += 1e-2 * rng.standard_normal((len(poses), 3)) / np.sqrt(3.0)
    return dict(poses=poses, H=J.T @ J, b=J.T @ rng.standard_normal(n - 3), T_lin=T, c=0.0)


def measure(Bs, reps, distinct, with_prior):
    """-> {B: {"without": ms, "with": ms, "slide": ms}} ("with" and "slide" only if asked)"""
    has_prior = load_binding()
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
        row = {"without": timed(solve, reset)}
        assert all(r.status == 0 and r.n_iter == ITERS for r in res)
        if with_prior and has_prior:
            priors = [synthetic_prior(base[k % len(base)], 100 + k % len(base)) for k in range(B)]
            batch.set_prior(priors)
            row["with"] = timed(solve, reset)
            assert all(r.status == 0 and r.n_iter == ITERS for r in res)
            batch.clear_prior()
            mark = np.concatenate([(np.arange(len(p["pose_fixed"])) ==
                                    np.flatnonzero(p["pose_fixed"] == 0)[0]).astype(np.uint8) for p in probs])

            def slide():
                solve()
                Hl, bl, kl, mres = batch.marginalize(mark, 1.0)
                T = batch.get_poses()
                batch.set_prior([dict(poses=kl[p], H=Hl[p], b=bl[p], T_lin=batch.poses_of(p, T)[kl[p]], c=0.0)
                                 for p in range(B)])
                solve()

            def reset_slide():
                batch.clear_prior()
                reset()
            row["slide"] = timed(slide, reset_slide)
            row["image_columns"] = batch.info()["image_columns"]
            row["lds_bytes"] = batch.info()["lds_bytes"]
        batch.close()
        out[B] = row
    return out


def child(lib, Bs, reps, distinct, with_prior):
    env = dict(os.environ)
    if lib:
        env["BA_HIP_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps), "--distinct", str(distinct),
           "--B"] + [str(b) for b in Bs] + (["--with-prior"] if with_prior else [])
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
    ap.add_argument("--with-prior", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.B, a.reps, a.distinct, a.with_prior)))
        return 0
    lines = []
    got = child(None, a.B, a.reps, a.distinct, True)
    for B in a.B:
        r = got[B]
        lines.append("B = %4d  %d iterations  without a prior %9.3f ms   with a K = 9 prior on every window %9.3f ms "
                     "(+%.1f %%)   slide (solve, marginalize, set the prior, solve) %9.3f ms   "
                     "(image %d columns, %d bytes of LDS)"
                     % (B, ITERS, r["without"], r["with"], 100.0 * (r["with"] / r["without"] - 1.0), r["slide"],
                        r["image_columns"], r["lds_bytes"]))
        print(lines[-1], flush=True)
    ok = True
    if a.parent_lib:
        par, new = [], []
        for _ in range(a.rounds):           # alternate, fresh processes
            par.append(child(os.path.abspath(a.parent_lib), a.B, a.reps, a.distinct, False))
            new.append(child(None, a.B, a.reps, a.distinct, False))
        for B in a.B:
            p = [x[B]["without"] for x in par]
            n = [x[B]["without"] for x in new]
            med = float(np.median(n))
            inside = med <= max(p)   # faster than the parent is no failure
            ok = ok and inside
            verdict = ("SLOWER than every run of the parent" if not inside else
                       "within the parent's spread" if med >= min(p) else
                       "not slower than the parent's runs (median below the parent's fastest)")
            lines.append("B = %4d  without a prior, %d fresh processes each, alternating: parent commit %s ms "
                         "(spread %.3f .. %.3f)   this commit %s ms   %s"
                         % (B, a.rounds, " ".join("%.3f" % v for v in p), min(p), max(p),
                            " ".join("%.3f" % v for v in n),
                            verdict))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("batch_prior_bench: windows of 10 poses (1 fixed) / 300 landmarks, stereo, sigma 0.5 px, %d LM "
                     "iterations; device time by hipEvents, best of %d\n" % (ITERS, a.reps))
            fh.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
