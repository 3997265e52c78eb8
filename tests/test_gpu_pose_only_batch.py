"""GPU tests of the batched 6-DoF pose-only solvers (ba_pose_only_{mono,stereo}6
_batch, one workgroup per problem).  A problem of <= 2048 points runs on one
workgroup in the single call too, so the batch must give it exactly the
single call's bits; larger problems agree to fp32 rounding."""
import os
import subprocess

import numpy as np
import pytest

from bundle_adjustment_solver_amd import scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import (BaProblem, Options,
                                                 PoseOnlyBundleAdjustmentSolver,
                                                 Summary)
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PO_KW = dict(max_iter=100, thr_step=1e-6, thr_cost=1e-6, huber=1.0, outlier=2.5)


def t12(T):
    T = np.asarray(T)
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]).astype(np.float32)


def scene(B, n_min, n_max, seed, stereo, **kw):
    kw.setdefault("pixel_sigma", 0.5)
    kw.setdefault("outlier_frac", 0.05)
    if stereo:
        kw.setdefault("right_missing_frac", 0.2)
    sc = scenes.pose_only_batch_scene(B, n_min, n_max, seed, stereo=stereo, **kw)
    sc["T12"] = np.stack([t12(T) for T in sc["T_init"]])
    if stereo:
        sc["Tlr12"] = np.stack([t12(T) for T in sc["T_lr"]])
    return sc


def run_batch(g, sc, stereo, opt, **kw):
    N = sc["X"].shape[0]
    if stereo:
        return g.pose_only_stereo6_batch(sc["offsets"], sc["X"], sc["uv"], sc["uv_right"],
                                         sc["intr"], sc["intr_r"], sc["Tlr12"], sc["T12"],
                                         np.ones(N, np.uint8), np.ones(N, np.uint8), opt, **kw)
    return g.pose_only_mono6_batch(sc["offsets"], sc["X"], sc["uv"], sc["intr"], sc["T12"],
                                   np.ones(N, np.uint8), opt, **kw)


def run_single(g, sc, b, stereo, opt, **kw):
    o = sc["offsets"]
    s = slice(o[b], o[b + 1])
    n = o[b + 1] - o[b]
    K = sc["intr"][b]
    if stereo:
        return g.pose_only_stereo6(sc["X"][s], sc["uv"][s], sc["uv_right"][s], K,
                                   sc["intr_r"][b], sc["Tlr12"][b], sc["T12"][b],
                                   np.ones(n, np.uint8), np.ones(n, np.uint8), opt, **kw)
    return g.pose_only_mono6(sc["X"][s], sc["uv"][s], *[float(v) for v in K], sc["T12"][b],
                             np.ones(n, np.uint8), opt, **kw)


MASKS = {False: ("mask",), True: ("mask_l", "mask_r")}


def assert_same(a, b, stereo, debug=True):
    assert np.array_equal(a["T12"], b["T12"])
    for k in MASKS[stereo]:
        assert np.array_equal(a[k], b[k]), k
    # (a NaN problem logs NaN rows: compared as arrays, NaN equal to NaN)
    assert len(a["rows"]) == len(b["rows"])
    assert np.array_equal(np.array(a["rows"], np.float32), np.array(b["rows"], np.float32),
                          equal_nan=True)
    assert a["n_iter"] == b["n_iter"] and a["converged"] == b["converged"]
    assert a["success"] == b["success"]
    if debug:
        assert np.array_equal(a["debug"], b["debug"], equal_nan=True)


@pytest.mark.parametrize("stereo", [False, True])
def test_bitwise_equal_to_single_calls(stereo, built):
    sc = scene(40, 64, 2048, seed=100 + stereo, stereo=stereo)
    g = BaProblem(0)
    opt = make_options(**PO_KW)
    res = run_batch(g, sc, stereo, opt, want_debug=True)
    assert len(res) == 40
    for b in range(40):
        one = run_single(g, sc, b, stereo, opt, want_debug=True)
        assert res[b]["status"] == 0
        assert_same(res[b], one, stereo)
    # and the batch really solves: near the true poses despite noise and outliers
    err = [np.abs(r["T12"] - t12(T)).max() for r, T in zip(res, sc["T_true"])]
    assert np.median(err) < 2e-2


@pytest.mark.parametrize("stereo", [False, True])
def test_large_problems_in_a_batch(stereo, built):
    """Above 2048 points the single call spreads a problem over several
    workgroups (another summation order): fp32 agreement, and the oracle
    tolerances of test_gpu_pose_only.py."""
    sc = scene(4, 5000, 20000, seed=7 + stereo, stereo=stereo, pixel_sigma=0.0,
               outlier_frac=0.0)
    g = BaProblem(0)
    res = run_batch(g, sc, stereo, make_options(**PO_KW))
    o = sc["offsets"]
    for b in range(4):
        one = run_single(g, sc, b, stereo, make_options(**PO_KW))
        assert np.abs(res[b]["T12"] - one["T12"]).max() < 1e-4
        s = slice(o[b], o[b + 1])
        n = o[b + 1] - o[b]
        K = sc["intr"][b]
        if stereo:
            ref = O.pose_only_stereo6(sc["X"][s], sc["uv"][s], sc["uv_right"][s], K, K,
                                      sc["T_lr"][b], sc["T_init"][b], np.ones(n, np.uint8),
                                      np.ones(n, np.uint8), O.make_options(**PO_KW))
        else:
            ref = O.pose_only_mono6(sc["X"][s], sc["uv"][s], K[0], K[1], K[2], K[3],
                                    sc["T_init"][b], np.ones(n, np.uint8),
                                    O.make_options(**PO_KW))
        assert ref["success"] and res[b]["success"]
        assert res[b]["converged"] == ref["converged"]
        assert abs(res[b]["n_iter"] - ref["n_iter"]) <= 1
        assert np.abs(res[b]["T12"] - ref["T12"]).max() < 1e-4
        for k in MASKS[stereo]:
            assert (res[b][k] != ref[k]).sum() <= max(2, n // 1000)


@pytest.mark.parametrize("stereo", [False, True])
def test_nan_problem_is_isolated(stereo, built):
    sc = scene(12, 64, 1500, seed=31 + stereo, stereo=stereo)
    g = BaProblem(0)
    opt = make_options(**PO_KW)
    clean = run_batch(g, sc, stereo, opt, want_debug=True)
    o = sc["offsets"]
    bad = 5
    sc["X"][o[bad]:o[bad] + 7] = np.nan
    res = run_batch(g, sc, stereo, opt, want_debug=True)
    assert res[bad]["status"] == 1 and not res[bad]["success"]
    assert np.array_equal(res[bad]["T12"], sc["T12"][bad])          # left unchanged
    one = run_single(g, sc, bad, stereo, opt, want_debug=True)
    assert not one["success"]
    assert_same(res[bad], one, stereo)
    for b in range(12):
        if b != bad:
            assert res[b]["status"] == 0
            assert_same(res[b], clean[b], stereo)


@pytest.mark.parametrize("stereo", [False, True])
def test_edge_cases(stereo, built):
    sc = scene(3, 100, 900, seed=51 + stereo, stereo=stereo)
    g = BaProblem(0)
    # B = 1
    one_sc = dict(sc)
    o = sc["offsets"]
    for k in ("X", "uv", "uv_right"):
        if k in sc:
            one_sc[k] = sc[k][:o[1]]
    one_sc["offsets"] = o[:2]
    for k in ("intr", "intr_r", "T12", "Tlr12"):
        if k in sc:
            one_sc[k] = sc[k][:1]
    opt = make_options(**PO_KW)
    assert_same(run_batch(g, one_sc, stereo, opt, want_debug=True)[0],
                run_single(g, sc, 0, stereo, opt, want_debug=True), stereo)
    # max_num_iterations = 0: pose unchanged, converged, no rows
    opt0 = make_options(**dict(PO_KW, max_iter=0))
    res = run_batch(g, sc, stereo, opt0)
    for b in range(3):
        one = run_single(g, sc, b, stereo, opt0)
        assert_same(res[b], one, stereo, debug=False)
        assert np.array_equal(res[b]["T12"], sc["T12"][b]) and res[b]["converged"]
        assert res[b]["rows"] == [] and res[b]["n_iter"] == 0
    # one iteration with zero thresholds: not converged, one row
    opt1 = make_options(**dict(PO_KW, max_iter=1, thr_step=0.0, thr_cost=0.0))
    res = run_batch(g, sc, stereo, opt1, want_debug=True)
    for b in range(3):
        assert_same(res[b], run_single(g, sc, b, stereo, opt1, want_debug=True), stereo)
    # run to run: the same bits
    a = run_batch(g, sc, stereo, opt, want_debug=True)
    b2 = run_batch(g, sc, stereo, opt, want_debug=True)
    for x, y in zip(a, b2):
        assert_same(x, y, stereo)


def test_oversubscribed_grid(built):
    """3000 workgroups of 1024 threads: far more than fit the device at once;
    no workgroup waits for another, so the launch drains."""
    sc = scene(3000, 100, 100, seed=77, stereo=False)
    g = BaProblem(0)
    opt = make_options(**PO_KW)
    res = run_batch(g, sc, False, opt)
    assert all(r["status"] == 0 for r in res)
    for b in (0, 1, 777, 1500, 2999):
        assert_same(res[b], run_single(g, sc, b, False, opt), False, debug=False)


@pytest.mark.parametrize("stereo", [False, True])
def test_tensor_path_on_a_side_stream(stereo, built):
    import torch
    sc = scene(24, 64, 2048, seed=91 + stereo, stereo=stereo)
    g = BaProblem(0)
    opt = make_options(**PO_KW)
    ref = run_batch(g, sc, stereo, opt, want_debug=True)
    dev = torch.device("cuda", 0)
    d = lambda a, t=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=t, device=dev)
    N = sc["X"].shape[0]
    args = dict(offsets=d(sc["offsets"], torch.int32), X3=d(sc["X"]), intr=d(sc["intr"]),
                T12=d(sc["T12"]), m=torch.ones(N, dtype=torch.uint8, device=dev))
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        if stereo:
            out = g.pose_only_stereo6_batch_tensors(
                args["offsets"], args["X3"], d(sc["uv"]), d(sc["uv_right"]), args["intr"],
                d(sc["intr_r"]), d(sc["Tlr12"]), args["T12"], args["m"], args["m"].clone(),
                opt, want_debug=True)
        else:
            out = g.pose_only_mono6_batch_tensors(args["offsets"], args["X3"], d(sc["uv"]),
                                                  args["intr"], args["T12"], args["m"], opt,
                                                  want_debug=True)
    s.synchronize()
    T = out["T12"].cpu().numpy()
    res = out["res"].cpu().numpy()
    rows = out["rows"].cpu().numpy()
    dbg = out["debug"].cpu().numpy()
    o = sc["offsets"]
    for b in range(24):
        r = ref[b]
        assert np.array_equal(T[b], r["T12"])
        assert list(res[b]) == [r["n_iter"], int(r["converged"]), len(r["rows"]), 0]
        assert [tuple(float(v) for v in x) for x in rows[b, :len(r["rows"])]] == r["rows"]
        assert np.array_equal(dbg[b, :r["n_iter"]], r["debug"])
        for k in MASKS[stereo]:
            assert np.array_equal(out[k][o[b]:o[b + 1]].cpu().numpy().astype(bool), r[k])
    # wrong dtype / device / layout
    with pytest.raises(ValueError, match="float32"):
        g.pose_only_mono6_batch_tensors(args["offsets"], args["X3"].double(), d(sc["uv"]),
                                        args["intr"], args["T12"], args["m"], opt)
    with pytest.raises(ValueError, match="int32"):
        g.pose_only_mono6_batch_tensors(args["offsets"].long(), args["X3"], d(sc["uv"]),
                                        args["intr"], args["T12"], args["m"], opt)
    with pytest.raises(ValueError, match="cuda"):
        g.pose_only_mono6_batch_tensors(args["offsets"], args["X3"].cpu(), d(sc["uv"]),
                                        args["intr"], args["T12"], args["m"], opt)
    with pytest.raises(ValueError, match="contiguous"):
        g.pose_only_mono6_batch_tensors(args["offsets"], args["X3"], d(sc["uv"]),
                                        args["intr"].t().contiguous().t(), args["T12"],
                                        args["m"], opt)


def _options():
    opt = Options()
    opt.iteration_handle.max_num_iterations = 100
    opt.convergence_handle.threshold_cost_change = 1e-6
    opt.convergence_handle.threshold_step_size = 1e-6
    opt.outlier_handle.threshold_huber_loss = 1.0
    opt.outlier_handle.threshold_outlier_rejection = 2.5
    return opt


def _frames(sc, stereo):
    o = sc["offsets"]
    fr = []
    for b in range(len(o) - 1):
        s = slice(o[b], o[b + 1])
        K = sc["intr"][b]
        if stereo:
            fr.append(dict(reference_position_list=list(sc["X"][s]),
                           matched_left_pixel_list=list(sc["uv"][s]),
                           matched_right_pixel_list=list(sc["uv_right"][s]),
                           fx_left=K[0], fy_left=K[1], cx_left=K[2], cy_left=K[3],
                           fx_right=K[0], fy_right=K[1], cx_right=K[2], cy_right=K[3],
                           left_to_right_pose=sc["T_lr"][b].astype(np.float64),
                           reference_to_current_left_pose=sc["T_init"][b].astype(np.float64),
                           mask_inlier_left=[], mask_inlier_right=[], summary=Summary()))
        else:
            fr.append(dict(reference_position_list=list(sc["X"][s]),
                           matched_pixel_list=list(sc["uv"][s]), fx=K[0], fy=K[1],
                           cx=K[2], cy=K[3],
                           reference_to_current_pose=sc["T_init"][b].astype(np.float64),
                           mask_inlier=[], summary=Summary()))
    return fr


@pytest.mark.parametrize("stereo", [False, True])
def test_mirror_batch_equals_single_mirror_calls(stereo, built):
    sc = scene(6, 200, 1500, seed=13 + stereo, stereo=stereo)
    s = PoseOnlyBundleAdjustmentSolver()
    frames = _frames(sc, stereo)
    ok = (s.Solve_Stereo_6Dof_Batch if stereo else s.Solve_Monocular_6Dof_Batch)(frames, _options())
    assert ok == [True] * 6
    for f, f1 in zip(frames, _frames(sc, stereo)):
        if stereo:
            assert s.Solve_Stereo_6Dof(*[f1[k] for k in (
                "reference_position_list", "matched_left_pixel_list", "matched_right_pixel_list",
                "fx_left", "fy_left", "cx_left", "cy_left", "fx_right", "fy_right", "cx_right",
                "cy_right", "left_to_right_pose", "reference_to_current_left_pose",
                "mask_inlier_left", "mask_inlier_right")], _options(), f1["summary"])
            pk, mks = "reference_to_current_left_pose", ("mask_inlier_left", "mask_inlier_right")
        else:
            assert s.Solve_Monocular_6Dof(*[f1[k] for k in (
                "reference_position_list", "matched_pixel_list", "fx", "fy", "cx", "cy",
                "reference_to_current_pose", "mask_inlier")], _options(), f1["summary"])
            pk, mks = "reference_to_current_pose", ("mask_inlier",)
        assert np.array_equal(f[pk], f1[pk])
        for mk in mks:
            assert f[mk] == f1[mk]
        a, b = f["summary"], f1["summary"]
        assert a.convergence_status_ == b.convergence_status_
        assert [(i.cost, i.cost_change, i.abs_step) for i in a.optimization_info_list_] == \
            [(i.cost, i.cost_change, i.abs_step) for i in b.optimization_info_list_]


@pytest.mark.parametrize("stereo", [False, True])
def test_cpp_facade_matches_python_mirror(stereo, tmp_path, built):
    sc = scene(5, 300, 1200, seed=71 + stereo, stereo=True)
    o = sc["offsets"]
    path = tmp_path / "frames.txt"
    with open(path, "w") as f:
        f.write("5 %d\n100 1e-6 1e-6 1.0 2.5\n" % int(stereo))
        for b in range(5):
            K = sc["intr"][b]
            f.write("%d %r %r %r %r\n" % (o[b + 1] - o[b], *[float(v) for v in K]))
            f.write(" ".join("%.9e" % v for v in t12(sc["T_lr"][b])) + "\n")
            f.write(" ".join("%.9e" % v for v in t12(sc["T_init"][b])) + "\n")
            rows = np.hstack([sc["X"], sc["uv"], sc["uv_right"]])[o[b]:o[b + 1]]
            for r in rows:
                f.write(" ".join("%.9e" % v for v in r) + "\n")
    r = subprocess.run([os.path.join(ROOT, "cpp", "build", "test_pose_only_batch"), str(path)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0 and "POSE-ONLY BATCH FACADE TEST PASSED" in r.stdout, r.stdout
    out, cur = [], None
    for line in r.stdout.splitlines():
        tag, _, rest = line.partition(" ")
        if tag == "frame":
            v = rest.split()
            cur = dict(success=int(v[2]), converged=int(v[4]), n_rows=int(v[6]), rows=[])
            out.append(cur)
        elif tag == "T12":
            cur["T12"] = np.array([float(x) for x in rest.split()], np.float32)
        elif tag == "row":
            cur["rows"].append([float(x) for x in rest.split()])
        elif tag in ("mask_l", "mask_r"):
            cur[tag] = np.array([c == "1" for c in rest.strip()], bool)
    assert len(out) == 5 and "all 1" in r.stdout
    if not stereo:
        sc = dict(sc)
        sc.pop("uv_right")
    frames = _frames(sc, stereo)
    s = PoseOnlyBundleAdjustmentSolver()
    (s.Solve_Stereo_6Dof_Batch if stereo else s.Solve_Monocular_6Dof_Batch)(frames, _options())
    for c, f in zip(out, frames):
        summ = f["summary"]
        assert c["success"] == 1 and c["converged"] == int(summ.convergence_status_)
        assert c["n_rows"] == len(summ.optimization_info_list_) == len(c["rows"])
        for a, b in zip(c["rows"], summ.optimization_info_list_):
            assert abs(a[0] - b.cost) <= 1e-6 * abs(b.cost)
            assert abs(a[2] - b.abs_step) <= 1e-6 * abs(b.abs_step)
        pose = f["reference_to_current_left_pose" if stereo else "reference_to_current_pose"]
        assert np.abs(c["T12"] - t12(pose)).max() < 1e-6
        assert np.array_equal(c["mask_l"], np.array(
            f["mask_inlier_left" if stereo else "mask_inlier"], bool))
        if stereo:
            assert np.array_equal(c["mask_r"], np.array(f["mask_inlier_right"], bool))


def test_single_kernel_resources_unchanged():
    """k_pose_only6<STEREO, false> keeps the single call's registers (128 VGPRs,
    4 VGPR spills); the batch instantiations do not spill more than that."""
    script = os.path.join(ROOT, "tools", "kernel_resources.sh")
    r = subprocess.run(["bash", script, "ba_pose_only.hip", "k_pose_only6"], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if "k_pose_only6" in l]
    assert len(lines) == 4, r.stdout
    for l in lines:
        assert "VGPR 128" in l, l
        if "Lb0EEEv" in l:              # <STEREO, false>: the single call
            assert "spill v4 " in l, l
