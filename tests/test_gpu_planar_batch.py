"""GPU tests of the batched planar 3-DoF pose-only solvers
(ba_pose_only_{mono,stereo}3_batch, one workgroup per problem).  A problem of
<= 2048 points runs on one workgroup in the single call too, so the batch must
give it exactly the single call's bits; larger problems agree to fp32 rounding
(checked against the numpy restatement tests/planar_pose_ref.py with the
tolerances of test_gpu_planar_pose_only.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import planar_pose_ref as R
from bundle_adjustment_solver_amd import _lib, scenes
from bundle_adjustment_solver_amd._lib import make_options
from bundle_adjustment_solver_amd.solver import (BaProblem, Options,
                                                 PoseOnlyBundleAdjustmentSolver,
                                                 Summary)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PO_KW = dict(max_iter=100, thr_step=1e-6, thr_cost=1e-6, huber=1.0, outlier=2.5)
MASKS = {False: ("mask",), True: ("mask_l", "mask_r")}


def t12(T):
    T = np.asarray(T)
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]).astype(np.float32)


def scene(B, n_min, n_max, seed, stereo, **kw):
    kw.setdefault("pixel_sigma", 0.5)
    kw.setdefault("outlier_frac", 0.05)
    if stereo:
        kw.setdefault("right_missing_frac", 0.2)
    sc = scenes.planar_pose_only_batch_scene(B, n_min, n_max, seed, stereo=stereo, **kw)
    for k in ("T_bc", "T_wl", "T_wc_init", "T_out_true") + (("T_lr",) if stereo else ()):
        sc[k + "12"] = np.stack([t12(T) for T in sc[k]])
    return sc


def run_batch(g, sc, stereo, opt, **kw):
    N = sc["X"].shape[0]
    if stereo:
        return g.pose_only_stereo3_batch(sc["offsets"], sc["X"], sc["uv"], sc["uv_right"],
                                         sc["intr"], sc["intr_r"], sc["T_bc12"], sc["T_lr12"],
                                         sc["T_wl12"], sc["T_wc_init12"], np.ones(N, np.uint8),
                                         np.ones(N, np.uint8), opt, **kw)
    return g.pose_only_mono3_batch(sc["offsets"], sc["X"], sc["uv"], sc["intr"], sc["T_bc12"],
                                   sc["T_wl12"], sc["T_wc_init12"], np.ones(N, np.uint8), opt,
                                   **kw)


def run_single(g, sc, b, stereo, opt, **kw):
    o = sc["offsets"]
    s = slice(o[b], o[b + 1])
    n = o[b + 1] - o[b]
    K = sc["intr"][b]
    if stereo:
        return g.pose_only_stereo3(sc["X"][s], sc["uv"][s], sc["uv_right"][s], K,
                                   sc["intr_r"][b], sc["T_bc12"][b], sc["T_lr12"][b],
                                   sc["T_wl12"][b], sc["T_wc_init12"][b], np.ones(n, np.uint8),
                                   np.ones(n, np.uint8), opt, **kw)
    return g.pose_only_mono3(sc["X"][s], sc["uv"][s], *[float(v) for v in K], sc["T_bc12"][b],
                             sc["T_wl12"][b], sc["T_wc_init12"][b], np.ones(n, np.uint8), opt,
                             **kw)


def assert_same(a, b, stereo, debug=True):
    assert np.array_equal(a["T12"], b["T12"], equal_nan=True)
    for k in MASKS[stereo]:
        assert np.array_equal(a[k], b[k]), k
    assert len(a["rows"]) == len(b["rows"])
    assert np.array_equal(np.array(a["rows"], np.float32), np.array(b["rows"], np.float32),
                          equal_nan=True)
    assert a["n_iter"] == b["n_iter"] and a["converged"] == b["converged"]
    assert a["success"] == b["success"]
    if debug:
        assert np.array_equal(a["debug"], b["debug"], equal_nan=True)


@pytest.fixture(scope="module")
def gpu(built):
    return BaProblem(0)


@pytest.mark.parametrize("stereo", [False, True])
def test_bitwise_equal_to_single_calls(gpu, stereo):
    sc = scene(40, 64, 2048, seed=200 + stereo, stereo=stereo)
    opt = make_options(**PO_KW)
    res = run_batch(gpu, sc, stereo, opt, want_debug=True)
    assert len(res) == 40
    for b in range(40):
        one = run_single(gpu, sc, b, stereo, opt, want_debug=True)
        assert res[b]["status"] == 0
        assert_same(res[b], one, stereo)
    # and the batch really solves: near the true poses despite noise and outliers
    err = [np.abs(r["T12"] - T).max() for r, T in zip(res, sc["T_out_true12"])]
    assert np.median(err) < 2e-2


@pytest.mark.parametrize("stereo", [False, True])
def test_large_problems_match_restatement(gpu, stereo):
    """Above 2048 points the single call spreads a problem over several
    workgroups; the batch keeps one.  Both agree with the numpy restatement to
    the tolerances of test_gpu_planar_pose_only.py."""
    sc = scene(4, 3000, 12000, seed=17 + stereo, stereo=stereo, outlier_frac=0.0)
    res = run_batch(gpu, sc, stereo, make_options(**PO_KW))
    o = sc["offsets"]
    for b in range(4):
        s = slice(o[b], o[b + 1])
        n = o[b + 1] - o[b]
        K = sc["intr"][b]
        kw = dict(PO_KW)
        if stereo:
            kw.update(uv_right=sc["uv_right"][s], T_lr=sc["T_lr"][b], mask_r=np.ones(n, bool),
                      intr_r=sc["intr_r"][b])
        ref = R.solve(sc["X"][s], sc["uv"][s], K[0], K[1], K[2], K[3], sc["T_bc"][b],
                      sc["T_wl"][b], sc["T_wc_init"][b], np.ones(n, bool), **kw)
        r = res[b]
        assert r["success"] and ref["success"] and r["status"] == 0
        assert r["converged"] == ref["converged"]
        assert abs(r["n_iter"] - ref["n_iter"]) <= 1
        assert np.abs(r["T12"] - ref["T12"]).max() < 1e-4
        k = min(len(r["rows"]), len(ref["rows"]))
        assert k >= 1
        for x, y in zip(r["rows"][:k], ref["rows"][:k]):
            assert abs(x[0] - y[0]) <= 1e-3 * max(abs(y[0]), 1e-3), (x, y)
            assert abs(x[2] - y[2]) <= 1e-3 * max(abs(y[2]), 1e-3), (x, y)
        for key in MASKS[stereo]:
            assert (r[key] != ref[key]).sum() <= max(2, n // 1000), key


@pytest.mark.parametrize("stereo", [False, True])
def test_nan_problem_is_isolated(gpu, stereo):
    sc = scene(12, 64, 1500, seed=41 + stereo, stereo=stereo)
    opt = make_options(**PO_KW)
    clean = run_batch(gpu, sc, stereo, opt, want_debug=True)
    o = sc["offsets"]
    bad = 5
    sc["uv"][o[bad] + 3, 0] = np.nan
    res = run_batch(gpu, sc, stereo, opt, want_debug=True)
    assert res[bad]["status"] == 1 and not res[bad]["success"]
    assert np.array_equal(res[bad]["T12"], sc["T_wc_init12"][bad])     # left unchanged
    one = run_single(gpu, sc, bad, stereo, opt, want_debug=True)
    assert not one["success"]
    assert_same(res[bad], one, stereo)
    for b in range(12):
        if b != bad:
            assert res[b]["status"] == 0
            assert_same(res[b], clean[b], stereo)
            assert_same(res[b], run_single(gpu, sc, b, stereo, opt, want_debug=True), stereo)


def _sub(sc, bs):
    """The problems `bs` of a batch scene as a batch scene of their own."""
    o = sc["offsets"]
    out = dict(sc)
    for k in ("X", "uv", "uv_right"):
        if k in sc:
            out[k] = np.concatenate([sc[k][o[b]:o[b + 1]] for b in bs])
    ns = [o[b + 1] - o[b] for b in bs]
    out["offsets"] = np.concatenate([[0], np.cumsum(ns)]).astype(np.int32)
    for k in ("intr", "intr_r", "T_bc12", "T_lr12", "T_wl12", "T_wc_init12"):
        if k in sc:
            out[k] = sc[k][list(bs)]
    return out


@pytest.mark.parametrize("stereo", [False, True])
def test_edge_cases(gpu, stereo):
    sc = scene(3, 100, 900, seed=61 + stereo, stereo=stereo)
    opt = make_options(**PO_KW)
    # B = 1
    assert_same(run_batch(gpu, _sub(sc, [1]), stereo, opt, want_debug=True)[0],
                run_single(gpu, sc, 1, stereo, opt, want_debug=True), stereo)
    # max_num_iterations = 0: every pose unchanged, converged, no rows
    opt0 = make_options(**dict(PO_KW, max_iter=0))
    res = run_batch(gpu, sc, stereo, opt0, want_debug=True)
    for b in range(3):
        assert_same(res[b], run_single(gpu, sc, b, stereo, opt0, want_debug=True), stereo)
        assert np.array_equal(res[b]["T12"], sc["T_wc_init12"][b]) and res[b]["converged"]
        assert res[b]["rows"] == [] and res[b]["n_iter"] == 0 and res[b]["status"] == 0
    # cap smaller than the iteration count: the first cap rows and debug poses
    opt1 = make_options(**dict(PO_KW, thr_step=0.0, thr_cost=0.0, max_iter=6))
    res = run_batch(gpu, sc, stereo, opt1, cap=2, want_debug=True)
    for b in range(3):
        one = run_single(gpu, sc, b, stereo, opt1, cap=2, want_debug=True)
        assert res[b]["n_iter"] == 6 and len(res[b]["rows"]) == 2 and len(res[b]["debug"]) == 2
        assert_same(res[b], one, stereo)
    # no rows and no debug poses wanted (null iters / debug_T12): the same poses
    full = run_batch(gpu, sc, stereo, opt)
    lib = _lib.load()
    N = sc["X"].shape[0]
    T = sc["T_wc_init12"].copy()
    ml, mr = np.ones(N, np.uint8), np.ones(N, np.uint8)
    resc = (_lib.BaPoResult * 3)()
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    off = sc["offsets"].ctypes.data_as(C.POINTER(C.c_int32))
    if stereo:
        rc = lib.ba_pose_only_stereo3_batch(
            gpu.h, 3, off, f(sc["X"]), f(sc["uv"]), f(sc["uv_right"]), f(sc["intr"]),
            f(sc["intr_r"]), f(sc["T_bc12"]), f(sc["T_lr12"]), f(sc["T_wl12"]), f(T), u8(ml),
            u8(mr), C.byref(opt), None, 7, resc, None)
    else:
        rc = lib.ba_pose_only_mono3_batch(
            gpu.h, 3, off, f(sc["X"]), f(sc["uv"]), f(sc["intr"]), f(sc["T_bc12"]),
            f(sc["T_wl12"]), f(T), u8(ml), C.byref(opt), None, 7, resc, None)
    assert rc == 0
    for b in range(3):
        assert np.array_equal(T[b], full[b]["T12"])
        assert (resc[b].n_iter, bool(resc[b].converged), resc[b].status) == \
            (full[b]["n_iter"], full[b]["converged"], 0)
    # a 1-point problem between two ordinary ones
    one_pt = _sub(sc, [0, 1, 2])
    o = sc["offsets"]
    keep = np.r_[o[0]:o[1], o[1]:o[1] + 1, o[2]:o[3]]
    for k in ("X", "uv", "uv_right"):
        if k in sc:
            one_pt[k] = sc[k][keep]
    one_pt["offsets"] = np.array([0, o[1], o[1] + 1, o[1] + 1 + o[3] - o[2]], np.int32)
    res = run_batch(gpu, one_pt, stereo, opt, want_debug=True)
    for b in range(3):
        assert_same(res[b], run_single(gpu, one_pt, b, stereo, opt, want_debug=True), stereo)
    # run to run: the same bits
    a = run_batch(gpu, sc, stereo, opt, want_debug=True)
    b2 = run_batch(gpu, sc, stereo, opt, want_debug=True)
    for x, y in zip(a, b2):
        assert_same(x, y, stereo)


def test_oversubscribed_grid(gpu):
    """3000 workgroups of 1024 threads: far more than fit the device at once;
    no workgroup waits for another, so the launch drains."""
    sc = scene(3000, 100, 100, seed=87, stereo=False)
    opt = make_options(**PO_KW)
    res = run_batch(gpu, sc, False, opt)
    assert all(r["status"] == 0 for r in res)
    for b in (0, 1, 777, 1500, 2999):
        assert_same(res[b], run_single(gpu, sc, b, False, opt), False, debug=False)


@pytest.mark.parametrize("stereo", [False, True])
def test_tensor_path_on_a_side_stream(gpu, stereo):
    import torch
    sc = scene(24, 64, 2048, seed=91 + stereo, stereo=stereo)
    opt = make_options(**PO_KW)
    ref = run_batch(gpu, sc, stereo, opt, want_debug=True)
    rec = BaProblem.planar_records(sc["T_bc12"], sc["T_wl12"], sc["T_wc_init12"],
                                   sc["T_lr12"] if stereo else None,
                                   sc["intr_r"] if stereo else None)
    dev = torch.device("cuda", 0)
    d = lambda a, t=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=t, device=dev)
    N = sc["X"].shape[0]
    off, X, K, T = d(sc["offsets"], torch.int32), d(sc["X"]), d(sc["intr"]), d(sc["T_wc_init12"])
    m = torch.ones(N, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        if stereo:
            out = gpu.pose_only_stereo3_batch_tensors(off, X, d(sc["uv"]), d(sc["uv_right"]), K,
                                                      d(rec), T, m, m.clone(), opt,
                                                      want_debug=True)
        else:
            out = gpu.pose_only_mono3_batch_tensors(off, X, d(sc["uv"]), K, d(rec), T, m, opt,
                                                    want_debug=True)
    s.synchronize()
    Tn = out["T12"].cpu().numpy()
    res = out["res"].cpu().numpy()
    rows = out["rows"].cpu().numpy()
    dbg = out["debug"].cpu().numpy()
    o = sc["offsets"]
    for b in range(24):
        r = ref[b]
        assert np.array_equal(Tn[b], r["T12"])
        assert list(res[b]) == [r["n_iter"], int(r["converged"]), len(r["rows"]), 0]
        assert [tuple(float(v) for v in x) for x in rows[b, :len(r["rows"])]] == r["rows"]
        assert np.array_equal(dbg[b, :r["n_iter"]], r["debug"])
        for k in MASKS[stereo]:
            assert np.array_equal(out[k][o[b]:o[b + 1]].cpu().numpy().astype(bool), r[k])
    # wrong dtype / record shape
    with pytest.raises(ValueError, match="float32"):
        gpu.pose_only_mono3_batch_tensors(off, X, d(sc["uv"]), K, d(rec).double(), T, m, opt)
    with pytest.raises(ValueError, match="52"):
        gpu.pose_only_mono3_batch_tensors(off, X, d(sc["uv"]), K, d(rec[:, :16]), T, m, opt)


def _options():
    opt = Options()
    opt.iteration_handle.max_num_iterations = 100
    opt.convergence_handle.threshold_cost_change = 1e-6
    opt.convergence_handle.threshold_step_size = 1e-6
    opt.outlier_handle.threshold_huber_loss = 1.0
    opt.outlier_handle.threshold_outlier_rejection = 2.5
    return opt


MONO_ARGS = ("world_position_list", "matched_pixel_list", "fx", "fy", "cx", "cy",
             "pose_base_to_camera", "pose_world_to_last", "pose_world_to_current",
             "mask_inlier")
STEREO_ARGS = ("world_position_list", "matched_left_pixel_list", "matched_right_pixel_list",
               "fx_left", "fy_left", "cx_left", "cy_left", "fx_right", "fy_right", "cx_right",
               "cy_right", "base_to_camera_pose", "left_to_right_pose", "world_to_last_pose",
               "world_to_current_pose", "mask_inlier_left", "mask_inlier_right")


def _frames(sc, stereo):
    o = sc["offsets"]
    fr = []
    f64 = lambda a: np.asarray(a, np.float64)
    for b in range(len(o) - 1):
        s = slice(o[b], o[b + 1])
        K = sc["intr"][b]
        if stereo:
            fr.append(dict(world_position_list=list(sc["X"][s]),
                           matched_left_pixel_list=list(sc["uv"][s]),
                           matched_right_pixel_list=list(sc["uv_right"][s]),
                           fx_left=K[0], fy_left=K[1], cx_left=K[2], cy_left=K[3],
                           fx_right=K[0], fy_right=K[1], cx_right=K[2], cy_right=K[3],
                           base_to_camera_pose=f64(sc["T_bc"][b]),
                           left_to_right_pose=f64(sc["T_lr"][b]),
                           world_to_last_pose=f64(sc["T_wl"][b]),
                           world_to_current_pose=f64(sc["T_wc_init"][b]).copy(),
                           mask_inlier_left=[], mask_inlier_right=[], summary=Summary()))
        else:
            fr.append(dict(world_position_list=list(sc["X"][s]),
                           matched_pixel_list=list(sc["uv"][s]), fx=K[0], fy=K[1],
                           cx=K[2], cy=K[3], pose_base_to_camera=f64(sc["T_bc"][b]),
                           pose_world_to_last=f64(sc["T_wl"][b]),
                           pose_world_to_current=f64(sc["T_wc_init"][b]).copy(),
                           mask_inlier=[], summary=Summary()))
    return fr


@pytest.mark.parametrize("stereo", [False, True])
def test_mirror_batch_equals_single_mirror_calls(stereo, built):
    sc = scene(6, 200, 1500, seed=23 + stereo, stereo=stereo)
    s = PoseOnlyBundleAdjustmentSolver()
    frames = _frames(sc, stereo)
    singles = _frames(sc, stereo)
    # one empty frame: left as is, mask emptied, success
    empty = dict(frames[0])
    for k in ("world_position_list", "matched_pixel_list", "matched_left_pixel_list",
              "matched_right_pixel_list"):
        if k in empty:
            empty[k] = []
    pk = "world_to_current_pose" if stereo else "pose_world_to_current"
    mks = ("mask_inlier_left", "mask_inlier_right") if stereo else ("mask_inlier",)
    empty.update({pk: frames[0][pk].copy(), "summary": Summary()}, **{mk: [True] for mk in mks})
    batch = (s.Solve_Stereo_Planar3Dof_Batch if stereo else
             s.Solve_Monocular_Planar3Dof_Batch)
    ok = batch(frames[:3] + [empty] + frames[3:], _options())
    assert ok == [True] * 7
    assert np.array_equal(empty[pk], _frames(sc, stereo)[0][pk])
    assert all(empty[mk] == [] for mk in mks)
    assert empty["summary"].convergence_status_ and not empty["summary"].optimization_info_list_
    assert s.GetDebugPoses() == []
    single = s.Solve_Stereo_Planar3Dof if stereo else s.Solve_Monocular_Planar3Dof
    for f, f1 in zip(frames, singles):
        assert single(*[f1[k] for k in (STEREO_ARGS if stereo else MONO_ARGS)], _options(),
                      f1["summary"])
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
            for key in ("T_bc12", "T_lr12", "T_wl12", "T_wc_init12"):
                f.write(" ".join("%.9e" % v for v in sc[key][b]) + "\n")
            rows = np.hstack([sc["X"], sc["uv"], sc["uv_right"]])[o[b]:o[b + 1]]
            for r in rows:
                f.write(" ".join("%.9e" % v for v in r) + "\n")
    r = subprocess.run([os.path.join(ROOT, "cpp", "build", "test_planar_batch"), str(path)],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0 and "PLANAR BATCH FACADE TEST PASSED" in r.stdout, r.stdout
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
    (s.Solve_Stereo_Planar3Dof_Batch if stereo else
     s.Solve_Monocular_Planar3Dof_Batch)(frames, _options())
    for c, f in zip(out, frames):
        summ = f["summary"]
        assert c["success"] == 1 and c["converged"] == int(summ.convergence_status_)
        assert c["n_rows"] == len(summ.optimization_info_list_) == len(c["rows"])
        for a, b in zip(c["rows"], summ.optimization_info_list_):
            assert abs(a[0] - b.cost) <= 1e-6 * abs(b.cost)
            assert abs(a[2] - b.abs_step) <= 1e-6 * abs(b.abs_step)
        pose = f["world_to_current_pose" if stereo else "pose_world_to_current"]
        assert np.abs(c["T12"] - t12(pose)).max() < 1e-6
        assert np.array_equal(c["mask_l"], np.array(
            f["mask_inlier_left" if stereo else "mask_inlier"], bool))
        if stereo:
            assert np.array_equal(c["mask_r"], np.array(f["mask_inlier_right"], bool))
