"""Batched 6-DoF pose-only solves (ba_pose_only_{mono,stereo}6_batch and their
_device variants): the parts that need no GPU — exports, bindings, host-side
argument checks, the mirror's size checks and the batch scene."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bundle_adjustment_solver_amd import _lib, scenes
from bundle_adjustment_solver_amd.solver import Options, PoseOnlyBundleAdjustmentSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ba_pose_only_mono6_batch", "ba_pose_only_stereo6_batch",
       "ba_pose_only_mono6_batch_device", "ba_pose_only_stereo6_batch_device"]


def test_batch_symbols_declared_exported_bound(built):
    src = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), "missing export: " + name
        assert name in _lib.SIGNATURES, name
    assert "ba_po_result" in src
    assert C.sizeof(_lib.BaPoResult) == 16


def _mono(lib, h, off, n_pts=8):
    B = len(off) - 1
    o = np.asarray(off, np.int32)
    X = np.zeros((n_pts, 3), np.float32)
    uv = np.zeros((n_pts, 2), np.float32)
    K = np.zeros((max(B, 1), 4), np.float32)
    T = np.zeros((max(B, 1), 12), np.float32)
    m = np.ones(n_pts, np.uint8)
    res = (_lib.BaPoResult * max(B, 1))()
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    return lib.ba_pose_only_mono6_batch(
        h, B, o.ctypes.data_as(C.POINTER(C.c_int32)), f(X), f(uv), f(K), f(T),
        m.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(_lib.make_options()), None, 0,
        res, None)


def _stereo(lib, h, off, n_pts=8):
    B = len(off) - 1
    o = np.asarray(off, np.int32)
    X = np.zeros((n_pts, 3), np.float32)
    uv = np.zeros((n_pts, 2), np.float32)
    K = np.zeros((max(B, 1), 4), np.float32)
    T = np.zeros((max(B, 1), 12), np.float32)
    m = np.ones(n_pts, np.uint8)
    res = (_lib.BaPoResult * max(B, 1))()
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    u8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
    return lib.ba_pose_only_stereo6_batch(
        h, B, o.ctypes.data_as(C.POINTER(C.c_int32)), f(X), f(uv), f(uv), f(K), f(K),
        f(T), f(T), u8(m), u8(m.copy()), C.byref(_lib.make_options()), None, 0, res, None)


@pytest.mark.parametrize("call,name", [(_mono, "ba_pose_only_mono6_batch"),
                                       (_stereo, "ba_pose_only_stereo6_batch")])
@pytest.mark.parametrize("off,what", [([0, 4, 8], "null handle"),
                                      ([1, 4, 8], "offsets[0]"),
                                      ([0, 4, 4, 8], "strictly increasing"),
                                      ([0, 5, 3], "strictly increasing"),
                                      ([0], "B must be")])
def test_host_checks_fail_before_any_device_use(call, name, off, what, built):
    lib = _lib.load()
    assert call(lib, None, off) < 0
    msg = lib.ba_last_error().decode()
    assert name in msg and what in msg, msg


def test_device_entry_points_refuse_null_handle(built):
    lib = _lib.load()
    opt = _lib.make_options()
    p = C.c_void_p(16)
    assert lib.ba_pose_only_mono6_batch_device(None, 2, p, p, p, p, p, p, C.byref(opt),
                                               None, 0, p, None, None) < 0
    assert b"ba_pose_only_mono6_batch_device" in lib.ba_last_error()
    assert lib.ba_pose_only_stereo6_batch_device(None, 2, p, p, p, p, p, p, p, p, p,
                                                 C.byref(opt), None, 0, p, None, None) < 0
    assert b"ba_pose_only_stereo6_batch_device" in lib.ba_last_error()


def test_right_camera_record_matches_single_call_expressions(built):
    """ba_right_camera_record = {intr_r, left_to_right^-1} in fp32, and the torch
    restatement used by the tensor path gives the same bits."""
    lib = _lib.load()
    sc = scenes.pose_only_batch_scene(3, 10, 20, seed=4, stereo=True)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for b in range(3):
        Tlr = np.concatenate([sc["T_lr"][b, :3, :3].reshape(9), sc["T_lr"][b, :3, 3]])
        Tlr = Tlr.astype(np.float32)
        out = np.zeros(16, np.float32)
        assert lib.ba_right_camera_record(f(sc["intr_r"][b].copy()), f(Tlr), f(out)) == 0
        R = Tlr[:9].reshape(3, 3).T
        assert np.array_equal(out[:4], sc["intr_r"][b])
        assert np.array_equal(out[4:13], R.reshape(9))
        t = -((R[:, 0] * Tlr[9] + R[:, 1] * Tlr[10]) + R[:, 2] * Tlr[11])
        assert np.array_equal(out[13:], t)
        import torch
        from bundle_adjustment_solver_amd.solver import BaProblem
        rec = BaProblem.right_camera_records(torch.from_numpy(sc["intr_r"][b:b + 1].copy()),
                                             torch.from_numpy(Tlr[None].copy()))
        assert np.array_equal(rec.numpy()[0], out)


def test_mirror_batch_size_mismatch_raises():
    """The per-frame size checks of the batch mirror methods come before any
    device use (an instance without a device problem behind it)."""
    s = PoseOnlyBundleAdjustmentSolver.__new__(PoseOnlyBundleAdjustmentSolver)
    s._p = None
    s.debug_poses_ = []
    sc = scenes.pose_only_batch_scene(2, 10, 12, seed=1, stereo=True)
    o = sc["offsets"]
    X, uv, ur = sc["X"], sc["uv"], sc["uv_right"]
    I = np.eye(4)
    good = dict(reference_position_list=list(X[o[0]:o[1]]),
                matched_pixel_list=list(uv[o[0]:o[1]]), fx=1, fy=1, cx=0, cy=0,
                reference_to_current_pose=I.copy(), mask_inlier=[])
    bad = dict(good, matched_pixel_list=list(uv[o[1]:o[2] - 1]),
               reference_position_list=list(X[o[1]:o[2]]))
    with pytest.raises(RuntimeError, match="current_pixel_list"):
        s.Solve_Monocular_6Dof_Batch([good, bad], Options())
    st = dict(reference_position_list=list(X[o[0]:o[1]]),
              matched_left_pixel_list=list(uv[o[0]:o[1]]),
              matched_right_pixel_list=list(ur[o[0]:o[1] - 1]),
              fx_left=1, fy_left=1, cx_left=0, cy_left=0, fx_right=1, fy_right=1,
              cx_right=0, cy_right=0, left_to_right_pose=I,
              reference_to_current_left_pose=I.copy(), mask_inlier_left=[],
              mask_inlier_right=[])
    with pytest.raises(RuntimeError, match="current_pixel_list"):
        s.Solve_Stereo_6Dof_Batch([st], Options())


def test_batch_scene_is_seeded():
    a = scenes.pose_only_batch_scene(6, 50, 200, seed=3, stereo=True, pixel_sigma=0.5,
                                     right_missing_frac=0.2, outlier_frac=0.05)
    b = scenes.pose_only_batch_scene(6, 50, 200, seed=3, stereo=True, pixel_sigma=0.5,
                                     right_missing_frac=0.2, outlier_frac=0.05)
    c = scenes.pose_only_batch_scene(6, 50, 200, seed=4, stereo=True)
    for k, v in a.items():
        assert np.array_equal(v, b[k]), k
    assert not np.array_equal(a["intr"], c["intr"])
    n = np.diff(a["offsets"])
    assert a["offsets"][0] == 0 and (n >= 50).all() and (n <= 200).all()
    assert a["X"].shape[0] == a["uv"].shape[0] == a["uv_right"].shape[0] == a["offsets"][-1]
    assert len(np.unique(a["intr"][:, 0])) == 6        # intrinsics vary per problem
    assert (a["uv_right"][a["right_missing"]] == -1).all()
