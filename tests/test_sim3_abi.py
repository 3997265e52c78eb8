"""Host tests of the Sim(3) pose graph's C ABI (ba_sim3_*; no GPU): the symbols and their ctypes
signatures, every refusal of ba_sim3_check and of ba_sim3_create (which validates before it
looks at the handle or touches a device), the calls on a null object, and the kernel table."""
import ctypes as C

import numpy as np
import pytest

from bundle_adjustment_solver_amd import _lib
from bundle_adjustment_solver_amd.solver import sim3_check


def test_symbols_and_signatures(built):
    lib = _lib.load()
    P, I32, U8, D, I64 = (C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double),
                          C.POINTER(C.c_int64))
    want = {
        "ba_sim3_create": [C.POINTER(P), P, C.c_int, D, U8, C.c_int64, I32, I32, D, D],
        "ba_sim3_update_values": [P, D, D, D],
        "ba_sim3_solve": [P, C.POINTER(_lib.BaOptions), C.POINTER(_lib.BaIterInfo), C.c_int, C.POINTER(C.c_int),
                          C.POINTER(C.c_int)],
        "ba_sim3_get_poses": [P, D],
        "ba_sim3_cost": [P, D],
        "ba_sim3_get_system": [P, D, D],
        "ba_sim3_factor_report": [P, D],
        "ba_sim3_info": [P, I64],
        "ba_sim3_last_ms": [P, D],
        "ba_sim3_check": [C.c_int, D, U8, C.c_int64, I32, I32, D, D],
    }
    for name, args in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    for name in ("ba_sim3_exp", "ba_sim3_log", "ba_sim3_adjoint"):
        fn = getattr(lib, name)
        assert fn.restype is None and list(fn.argtypes) == [D, D], name
    assert lib.ba_sim3_destroy.restype is None
    lib.ba_sim3_destroy(None)
    # null object: refused on the host, nothing touches a device
    assert lib.ba_sim3_update_values(None, None, None, None) == -1
    assert lib.ba_sim3_solve(None, None, None, 0, None, None) == -1
    assert lib.ba_sim3_get_poses(None, None) == -1
    assert lib.ba_sim3_cost(None, None) == -1
    assert lib.ba_sim3_get_system(None, None, None) == -1
    assert lib.ba_sim3_factor_report(None, None) == -1
    assert lib.ba_sim3_info(None, None) == -1
    assert lib.ba_sim3_last_ms(None, None) == -1
    names = [lib.ba_kernel_name(k).decode() for k in range(lib.ba_kernel_count())]
    assert {"k_s3_lin", "k_s3_assemble", "k_s3_trial"} <= set(names) and len(set(names)) == len(names)


def _good():
    """5 poses, poses 0 and 1 fixed, 5 factors naming every optimisable pose"""
    rng = np.random.default_rng(1)
    S = np.tile(np.r_[np.eye(3).reshape(9), np.zeros(3), 1.0], (5, 1))
    S[:, 9] = np.arange(5)
    fx = np.array([1, 1, 0, 0, 0], np.uint8)
    j = np.array([2, 3, 4, 0, 4], np.int32)
    k = np.array([1, 2, 3, 3, 2], np.int32)
    Z = np.tile(np.r_[np.eye(3).reshape(9), np.zeros(3), 1.0], (5, 1))
    J = rng.standard_normal((5, 9, 7))
    return S, fx, j, k, Z, np.einsum("fab,fac->fbc", J, J)


def _call(create, S, fx, j, k, Z, Om, n_pose=None, n_rel=None):
    lib = _lib.load()
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
    S, Z, Om, j, k = f64(S), f64(Z), f64(Om), i32(j), i32(k)
    fx = None if fx is None else np.ascontiguousarray(fx, np.uint8)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    up = None if fx is None else fx.ctypes.data_as(C.POINTER(C.c_uint8))
    n_pose = S.shape[0] if n_pose is None else n_pose
    n_rel = len(j) if n_rel is None else n_rel
    if create:   # no handle: every refusal below comes before the handle is looked at
        out = C.c_void_p()
        rc = lib.ba_sim3_create(C.byref(out), None, n_pose, dp(S), up, n_rel, ip(j), ip(k), dp(Z), dp(Om))
        assert not out.value
    else:
        rc = lib.ba_sim3_check(n_pose, dp(S), up, n_rel, ip(j), ip(k), dp(Z), dp(Om))
    return rc, (lib.ba_last_error() or b"").decode()


def test_accepts_a_valid_graph(built):
    S, fx, j, k, Z, Om = _good()
    assert _call(False, S, fx, j, k, Z, Om)[0] == 0
    assert _call(False, S, None, j, k, Z, Om)[0] == 0    # no fixed pose: not refused
    sim3_check(S, fx, dict(j=j, k=k, Z=Z, Omega=Om))
    # a valid graph reaches the handle check of create, and only that
    rc, msg = _call(True, S, fx, j, k, Z, Om)
    assert rc == -1 and msg == "ba_sim3_create: null handle"


@pytest.mark.parametrize("create", [False, True])
@pytest.mark.parametrize("what,where", [
    ("j_high", "pose j = 5 out of range (factor 2)"),
    ("k_low", "pose k = -2 out of range (factor 0)"),
    ("same", "j == k: a factor needs two distinct poses (factor 2)"),
    ("both_fixed", "both poses are fixed (factor 3)"),
    ("Z_nan", "Z is not finite (factor 1)"),
    ("Z_rot_nan", "the rotation of Z is not finite (factor 2)"),
    ("Z_scale_zero", "the scale of Z must be > 0 (factor 3)"),
    ("Z_scale_neg", "the scale of Z must be > 0 (factor 0)"),
    ("Z_scale_inf", "the scale of Z is not finite (factor 4)"),
    ("Om_inf", "Omega is not finite (factor 4)"),
    ("S_nan", "S_jw is not finite (pose 3)"),
    ("S_rot_inf", "the rotation of S_jw is not finite (pose 1)"),
    ("S_scale_zero", "the scale of S_jw must be > 0 (pose 2)"),
    ("S_scale_neg", "the scale of S_jw must be > 0 (pose 4)"),
    ("S_scale_nan", "the scale of S_jw is not finite (pose 0)"),
    ("unnamed", "pose 4 is optimisable but no factor names it"),
    ("no_pose", "n_pose must be >= 1"),
    ("no_factor", "n_rel must be >= 1: a pose graph needs a factor"),
    ("null_Z", "null factor array (factor 0)"),
    ("null_Om", "null factor array (factor 0)"),
    ("null_j", "null factor array (factor 0)"),
    ("null_S", "null pose array"),
])
def test_refusals_name_the_factor_or_the_pose(built, create, what, where):
    S, fx, j, k, Z, Om = _good()
    kw = {}
    if what == "j_high":
        j[2] = 5
    elif what == "k_low":
        k[0] = -2
    elif what == "same":
        k[2] = j[2]
    elif what == "both_fixed":
        j[3], k[3] = 0, 1
    elif what == "Z_nan":
        Z[1, 10] = np.nan
    elif what == "Z_rot_nan":
        Z[2, 4] = np.nan
    elif what == "Z_scale_zero":
        Z[3, 12] = 0.0
    elif what == "Z_scale_neg":
        Z[0, 12] = -1.0
    elif what == "Z_scale_inf":
        Z[4, 12] = np.inf
    elif what == "Om_inf":
        Om[4, 0, 6] = np.inf
    elif what == "S_nan":
        S[3, 11] = np.nan
    elif what == "S_rot_inf":
        S[1, 0] = np.inf
    elif what == "S_scale_zero":
        S[2, 12] = 0.0
    elif what == "S_scale_neg":
        S[4, 12] = -2.0
    elif what == "S_scale_nan":
        S[0, 12] = np.nan
    elif what == "unnamed":
        j[2], k[2] = 2, 3   # factors 2 and 4 become (2, 3) and (3, 2): nobody names pose 4
        j[4], k[4] = 3, 2
    elif what == "no_pose":
        kw["n_pose"] = 0
    elif what == "no_factor":
        kw["n_rel"] = 0
    elif what == "null_Z":
        Z = None
    elif what == "null_Om":
        Om = None
    elif what == "null_j":
        j, kw["n_rel"] = None, 5
    elif what == "null_S":
        S, kw["n_pose"] = None, 5
    rc, msg = _call(create, S, fx, j, k, Z, Om, **kw)
    assert rc == -1 and msg == "ba_sim3_create: " + where, msg


def test_python_wrapper_refuses_without_a_device(built):
    S, fx, j, k, Z, Om = _good()
    Z[2, 12] = -0.5
    with pytest.raises(_lib.BaError, match="the scale of Z must be > 0 \\(factor 2\\)"):
        sim3_check(S, fx, dict(j=j, k=k, Z=Z, Omega=Om))
