"""Host-side contract of ba_point_only (no GPU): every refusal of ba_point_only_check, the
edge structures it accepts, and the refusals ba_point_only itself makes before it touches
a device (it is called with a NULL handle, which is the last thing it checks)."""
import ctypes as C

import numpy as np
import pytest

from bundle_adjustment_solver_amd import _lib
from bundle_adjustment_solver_amd._lib import BaError, BaPointResult, make_options
from bundle_adjustment_solver_amd.solver import (_point_only_structure, point_only_check,
                                                 point_only_team)


@pytest.fixture(scope="module")
def lib(built):
    return _lib.load()


def structure(counts, n_cam=2, n_pose=3, seed=0):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(off[-1])
    return off, rng.integers(0, n_cam, max(n, 1)).astype(np.int32), rng.integers(0, n_pose, max(n, 1)).astype(np.int32)


def refused(fn, *args):
    with pytest.raises(BaError) as e:
        fn(*args)
    return str(e.value)


def test_accepted_structures(lib):
    for counts in ([5], [0], [1], [2, 0, 3], [0, 0, 0], [16, 17, 33, 1, 0, 8], [0, 4], [4, 0]):
        off, cam, pose = structure(counts)
        assert point_only_check(2, 3, len(counts), off, cam, pose)
    off, cam, pose = structure([3, 3], n_cam=1, n_pose=1)
    assert point_only_check(1, 1, 2, off, cam, pose)


def test_refusals_of_the_check(lib):
    off, cam, pose = structure([2, 0, 3])
    assert "n_cam" in refused(point_only_check, 0, 3, 3, off, cam, pose)
    assert "n_pose" in refused(point_only_check, 2, 0, 3, off, cam, pose)
    bad = off.copy()
    bad[0] = 1
    assert "obs_off[0]" in refused(point_only_check, 2, 3, 3, bad, cam, pose)
    bad = off.copy()
    bad[2] = 1                                     # 0 2 1 5
    assert "decreases at landmark 1" in refused(point_only_check, 2, 3, 3, bad, cam, pose)
    for arr, what, hi in ((cam, "camera", 2), (pose, "pose", 3)):
        for v in (-1, hi):
            b = arr.copy()
            b[3] = v
            a = (b, pose) if what == "camera" else (cam, b)
            msg = refused(point_only_check, 2, 3, 3, off, *a)
            assert what in msg and "observation 3" in msg and "landmark 2" in msg, msg
    # n_pt < 1 and NULL pointers, through the C symbol itself
    I64, I32 = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    po, pc, pp = off.ctypes.data_as(I64), cam.ctypes.data_as(I32), pose.ctypes.data_as(I32)
    for args, word in (((2, 3, 0, po, pc, pp), "n_pt"), ((2, 3, 3, None, pc, pp), "null obs_off"),
                       ((2, 3, 3, po, None, pp), "null obs_cam"), ((2, 3, 3, po, pc, None), "null obs_cam")):
        assert lib.ba_point_only_check(*args) == -1
        assert word in lib.ba_last_error().decode()
    assert lib.ba_point_only_check(2, 3, 3, po, pc, pp) == 0


def test_the_call_refuses_before_it_needs_a_gpu(lib):
    off, cam, pose = structure([2, 0, 3])
    D = C.POINTER(C.c_double)
    intr, Tc, Tp = np.ones((2, 4)), np.zeros((2, 12)), np.zeros((3, 12))
    uv, X = np.zeros((5, 2)), np.zeros((3, 3))
    opt, res = make_options(), (BaPointResult * 3)()
    dp = lambda a: a.ctypes.data_as(D)
    good = [None, 2, dp(intr), dp(Tc), 3, dp(Tp), 3, off.ctypes.data_as(C.POINTER(C.c_int64)),
            cam.ctypes.data_as(C.POINTER(C.c_int32)), pose.ctypes.data_as(C.POINTER(C.c_int32)), dp(uv),
            None, dp(X), C.byref(opt), None, 0, res]
    for k, word in ((2, "null pointer"), (3, "null pointer"), (5, "null pointer"), (10, "null pointer"),
                    (12, "null pointer"), (13, "null pointer"), (16, "null pointer"), (7, "null obs_off"),
                    (8, "null obs_cam"), (9, "null obs_cam")):
        a = list(good)
        a[k] = None
        assert lib.ba_point_only(*a) == -1
        assert word in lib.ba_last_error().decode(), (k, lib.ba_last_error())
    a = list(good)
    a[15] = -1
    assert lib.ba_point_only(*a) == -1 and "cap" in lib.ba_last_error().decode()
    a = list(good)
    a[6] = 0
    assert lib.ba_point_only(*a) == -1 and "n_pt" in lib.ba_last_error().decode()
    cam_bad = cam.copy()
    cam_bad[4] = 2
    a = list(good)
    a[8] = cam_bad.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.ba_point_only(*a) == -1
    assert "observation 4 (landmark 2)" in lib.ba_last_error().decode()
    # everything else in order: the handle is what is missing
    assert lib.ba_point_only(*good) == -1 and "null handle" in lib.ba_last_error().decode()
    assert np.array_equal(X, np.zeros((3, 3)))


def test_team_width_and_the_python_structure(lib):
    w = point_only_team(0)
    assert w in (8, 16)
    assert point_only_team(8) == 8 and point_only_team(0) == 8
    assert point_only_team(16) == 16
    assert "8 or 16" in refused(point_only_team, 12)
    assert point_only_team(w) == w
    # observations in any order: stable sort by point, offsets with empty landmarks
    pt = np.array([2, 0, 2, 0, 3, 2])
    off, cam, pose, uv, order = _point_only_structure("t", 5, np.arange(6), np.arange(6) + 10, pt,
                                                      np.arange(12.0).reshape(6, 2))
    assert off.tolist() == [0, 2, 2, 5, 6, 6] and order.tolist() == [1, 3, 0, 2, 5, 4]
    assert cam.tolist() == [1, 3, 0, 2, 5, 4] and pose.tolist() == [11, 13, 10, 12, 15, 14]
    assert uv[:, 0].tolist() == [2, 6, 0, 4, 10, 8]
    with pytest.raises(ValueError):
        _point_only_structure("t", 3, np.arange(6), np.arange(6), pt, np.zeros((6, 2)))
