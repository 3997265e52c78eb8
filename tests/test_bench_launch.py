"""bench.py --gpus N started as a PLAIN python command (no torchrun): the script
must start its N ranks itself, as child processes, before anything touches the
GPU, relay rank 0's single JSON line and the ranks' exit code.

* without a GPU (this container): the ranks are started, form their process group
  and then fail LOUDLY at ba_create — the product has no CPU path — and the parent
  exits non-zero;
* on the GPU box: two ranks rehearse on the one card (BA_BENCH_BACKEND=gloo: RCCL
  refuses two ranks on one device; the exchange is staged through the host) and
  the line must name 2 ranks seen by the communicator; the strong-scaling run
  must reproduce the one-rank trajectory, the weak run doubles the landmarks.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def run_bench(args, extra_env=None, timeout=900):
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    env.pop("LOCAL_RANK", None)
    env.update(extra_env or {})
    return subprocess.run([sys.executable, BENCH] + args, env=env, cwd=ROOT,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=timeout)


def json_lines(text):
    out = []
    for line in text.splitlines():
        line = line.strip()
        if line.startswith("{") and line.endswith("}"):
            try:
                out.append(json.loads(line))
            except ValueError:
                pass
    return out


def _has_gpu():
    import torch
    return torch.cuda.device_count() > 0


def test_self_launch_without_gpu_fails_loudly(built):
    if _has_gpu():
        pytest.skip("a GPU is present: covered by the gpu-marked tests below")
    r = run_bench(["--gpus", "2", "--scale", "0.02", "--steps", "2", "--warmup", "1",
                   "--no-cpu-baseline"], {"BA_BENCH_BACKEND": "gloo"})
    assert r.returncode != 0
    assert not json_lines(r.stdout)              # no result line without a GPU
    # both ranks were started and both refused to run without the HIP device
    assert r.stderr.count("no HIP device available (the HIP path has no CPU fallback)") >= 2
    assert "[rank0]" in r.stderr and "[rank1]" in r.stderr


@pytest.mark.gpu
def test_plain_python_gpus2_rehearsal_prints_one_json_line(built):
    common = ["--scale", "0.02", "--steps", "6", "--warmup", "2", "--no-cpu-baseline",
              "--no-roofline", "--config", "C3"]
    one = run_bench(["--gpus", "1"] + common)
    assert one.returncode == 0, one.stderr[-2000:]
    l1 = json_lines(one.stdout)
    assert len(l1) == 1
    two = run_bench(["--gpus", "2"] + common, {"BA_BENCH_BACKEND": "gloo"})
    assert two.returncode == 0, two.stderr[-2000:]
    l2 = json_lines(two.stdout)
    assert len(l2) == 1, two.stdout
    a, b = l1[0], l2[0]
    assert b["n_gpus"] == 2 and b["n_ranks_seen"] == 2 and b["scaling"] == "strong"
    assert "REHEARSAL" in b["config"]["parallelism"]
    assert a["n_gpus"] == 1 and a["n_ranks_seen"] == 1
    assert b["config"]["n_observations"] == a["config"]["n_observations"]
    # the same problem, the same LM trajectory: sharding only permutes summation order
    assert abs(a["final_cost"] - b["final_cost"]) <= 1e-9 * abs(a["final_cost"])
    weak = run_bench(["--gpus", "2", "--weak"] + common, {"BA_BENCH_BACKEND": "gloo"})
    assert weak.returncode == 0, weak.stderr[-2000:]
    lw = json_lines(weak.stdout)
    assert len(lw) == 1
    w = lw[0]
    assert w["scaling"] == "weak" and w["n_ranks_seen"] == 2
    assert w["config"]["n_observations"] == 2 * a["config"]["n_observations"]
    assert w["config"]["n_opt_poses"] == a["config"]["n_opt_poses"]


@pytest.mark.gpu
def test_one_rank_rccl_exchange_path_of_the_bench(built):
    """What a one-GPU box can run of the multi-GPU bench with REAL RCCL: one rank,
    `nccl` process group, the library's own RCCL communicator (ba_rccl_*, hook called
    from C++), the sharded iteration (separate control kernel, non-direct
    k_schur_final + k_scatter) and the final landmark gather — same trajectory as the
    plain single-GPU run of the same problem."""
    common = ["--gpus", "1", "--scale", "0.05", "--config", "C3", "--steps", "6", "--warmup", "2",
              "--no-cpu-baseline", "--no-roofline"]
    plain = run_bench(common)
    assert plain.returncode == 0, plain.stderr[-2000:]
    forced = run_bench(common + ["--force-exchange"])
    assert forced.returncode == 0, forced.stderr[-3000:]
    a, b = json_lines(plain.stdout), json_lines(forced.stdout)
    assert len(a) == 1 and len(b) == 1
    a, b = a[0], b[0]
    assert "RCCL all-reduce issued by libba_hip.so" in b["config"]["exchange"]
    assert b["n_ranks_seen"] == 1 and "gather_points_ms" in b
    assert abs(a["final_cost"] - b["final_cost"]) <= 1e-9 * abs(a["final_cost"])


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float64_arrays_within_the_limit(tmp_path, monkeypatch):
    """--dump-outputs: the poses and points as float64 .npy files; past the size
    limit the points become a seeded sample of rows, the same rows on every call,
    named by points_sample_rows.npy."""
    import numpy as np
    bench = _bench_module()
    rng = np.random.default_rng(3)
    poses, points = rng.standard_normal((7, 12)), rng.standard_normal((5000, 3))
    bench.dump_outputs(str(tmp_path / "a"), poses, points)
    assert sorted(f.name for f in (tmp_path / "a").iterdir()) == ["points.npy", "poses.npy"]
    got = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("poses", "points")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["poses"], poses) and np.array_equal(got["points"], points)

    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", (1 << 20) + 64 * 1024)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), poses, points)
    total = sum(f.stat().st_size for f in (tmp_path / "b").iterdir())
    assert total <= bench.DUMP_LIMIT_BYTES
    sel = np.load(str(tmp_path / "b" / "points_sample_rows.npy"))
    sub = np.load(str(tmp_path / "b" / "points.npy"))
    assert sel.dtype == np.float64 and 0 < sel.size < points.shape[0]
    assert np.array_equal(sub, points[sel.astype(np.int64)])
    for n in ("points", "points_sample_rows"):
        assert np.array_equal(np.load(str(tmp_path / "b" / (n + ".npy"))),
                              np.load(str(tmp_path / "c" / (n + ".npy"))))


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_run_dumps_the_same_outputs(built, tmp_path):
    """A plain run times --steps steps and prints the headline only; --full adds the
    instrumented pass and the CPU baseline AFTER the dump, so both runs dump the
    same outputs of the timed path (no floating-point atomics: bit-identical)."""
    import numpy as np
    common = ["--gpus", "1", "--config", "C1", "--steps", "5", "--warmup", "2"]
    plain = run_bench(common + ["--dump-outputs", str(tmp_path / "plain")])
    assert plain.returncode == 0, plain.stderr[-2000:]
    full = run_bench(common + ["--full", "--dump-outputs", str(tmp_path / "full")])
    assert full.returncode == 0, full.stderr[-2000:]
    (a,), (b,) = json_lines(plain.stdout), json_lines(full.stdout)
    for line in (a, b):
        assert line["metric"] == "lm_iterations_per_sec" and line["unit"] == "it/s"
        assert line["dtype"] == "f64" and line["higher_is_better"] is True
        assert line["steps"] == 5 and line["warmup"] == 2 and line["ms_per_step"] > 0
        assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-9 * line["value"]
    for key in ("stage_ms", "roofline", "end_to_end_solve_s", "cpu_baseline"):
        assert key not in a and key in b, key
    for name in ("poses", "points"):
        x = np.load(str(tmp_path / "plain" / (name + ".npy")))
        y = np.load(str(tmp_path / "full" / (name + ".npy")))
        assert x.dtype == np.float64 and np.array_equal(x, y), name
        assert np.isfinite(x).all(), name
    assert np.load(str(tmp_path / "plain" / "points.npy")).shape[1] == 3


@pytest.mark.gpu
def test_long_thresholds_off_run_dumps_finite_outputs(built, tmp_path):
    """The headline workload timed far past convergence (the thresholds are off):
    a weakly constrained landmark runs away and the iteration records go
    non-finite, but rejected trial points never reach the parameters, so the
    dumped poses and points stay finite."""
    import numpy as np
    r = run_bench(["--gpus", "1", "--steps", "1500", "--warmup", "5",
                   "--dump-outputs", str(tmp_path)], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    (line,) = json_lines(r.stdout)
    assert line["steps"] == 1500
    assert not np.isfinite(line["final_cost"])       # the run-away regime is reached
    for name in ("poses", "points"):
        assert np.isfinite(np.load(str(tmp_path / (name + ".npy")))).all(), name
