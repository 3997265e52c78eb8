"""Host tests of the pose-graph optimisation (ba_pgraph_*; no GPU): the symbols and their ctypes
signatures, every refusal of ba_pgraph_check and of ba_pgraph_create (which validates before it
looks at the handle or touches a device), and the calls on a null object."""
import ctypes as C

import numpy as np
import pytest

from bundle_adjustment_solver_amd import _lib
from bundle_adjustment_solver_amd.solver import pgraph_check


def test_symbols_and_signatures(built):
    lib = _lib.load()
    P, I32, U8, D, I64 = (C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_double),
                          C.POINTER(C.c_int64))
    want = {
        "ba_pgraph_create": [C.POINTER(P), P, C.c_int, D, U8, C.c_int64, I32, I32, D, D],
        "ba_pgraph_update_values": [P, D, D, D],
        "ba_pgraph_solve": [P, C.POINTER(_lib.BaOptions), C.POINTER(_lib.BaIterInfo), C.c_int, C.POINTER(C.c_int),
                            C.POINTER(C.c_int)],
        "ba_pgraph_get_poses": [P, D],
        "ba_pgraph_cost": [P, D],
        "ba_pgraph_get_system": [P, D, D],
        "ba_pgraph_info": [P, I64],
        "ba_pgraph_last_ms": [P, D],
        "ba_pgraph_check": [C.c_int, D, U8, C.c_int64, I32, I32, D, D],
    }
    for name, args in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    assert lib.ba_pgraph_destroy.restype is None
    lib.ba_pgraph_destroy(None)
    # null object: refused on the host, nothing touches a device
    assert lib.ba_pgraph_update_values(None, None, None, None) == -1
    assert lib.ba_pgraph_solve(None, None, None, 0, None, None) == -1
    assert lib.ba_pgraph_get_poses(None, None) == -1
    assert lib.ba_pgraph_cost(None, None) == -1
    assert lib.ba_pgraph_get_system(None, None, None) == -1
    assert lib.ba_pgraph_info(None, None) == -1
    assert lib.ba_pgraph_last_ms(None, None) == -1
    names = [lib.ba_kernel_name(k).decode() for k in range(lib.ba_kernel_count())]
    assert names[-4:] == ["k_pg_lin", "k_pg_assemble", "k_pg_trial", "k_pg_control"]


def _good():
    """5 poses, poses 0 and 1 fixed, 5 factors naming every optimisable pose"""
    rng = np.random.default_rng(1)
    T = np.tile(np.r_[np.eye(3).reshape(9), np.zeros(3)], (5, 1))
    T[:, 9] = np.arange(5)
    fx = np.array([1, 1, 0, 0, 0], np.uint8)
    j = np.array([2, 3, 4, 0, 4], np.int32)
    k = np.array([1, 2, 3, 3, 2], np.int32)
    Z = np.tile(np.r_[np.eye(3).reshape(9), np.zeros(3)], (5, 1))
    J = rng.standard_normal((5, 8, 6))
    return T, fx, j, k, Z, np.einsum("fab,fac->fbc", J, J)


def _call(create, T, fx, j, k, Z, Om, n_pose=None, n_rel=None):
    lib = _lib.load()
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, np.float64)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)
    T, Z, Om, j, k = f64(T), f64(Z), f64(Om), i32(j), i32(k)
    fx = None if fx is None else np.ascontiguousarray(fx, np.uint8)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
    up = None if fx is None else fx.ctypes.data_as(C.POINTER(C.c_uint8))
    n_pose = T.shape[0] if n_pose is None else n_pose
    n_rel = len(j) if n_rel is None else n_rel
    if create:   # no handle: every refusal below comes before the handle is looked at
        out = C.c_void_p()
        rc = lib.ba_pgraph_create(C.byref(out), None, n_pose, dp(T), up, n_rel, ip(j), ip(k), dp(Z), dp(Om))
        assert not out.value
    else:
        rc = lib.ba_pgraph_check(n_pose, dp(T), up, n_rel, ip(j), ip(k), dp(Z), dp(Om))
    return rc, (lib.ba_last_error() or b"").decode()


def test_accepts_a_valid_graph(built):
    T, fx, j, k, Z, Om = _good()
    assert _call(False, T, fx, j, k, Z, Om)[0] == 0
    assert _call(False, T, None, j, k, Z, Om)[0] == 0    # no fixed pose: not refused
    pgraph_check(T, fx, dict(j=j, k=k, Z=Z, Omega=Om))
    # a valid graph reaches the handle check of create, and only that
    rc, msg = _call(True, T, fx, j, k, Z, Om)
    assert rc == -1 and msg == "ba_pgraph_create: null handle"


@pytest.mark.parametrize("create", [False, True])
@pytest.mark.parametrize("what,where", [
    ("j_high", "pose j = 5 out of range (factor 2)"),
    ("k_low", "pose k = -2 out of range (factor 0)"),
    ("same", "j == k: a factor needs two distinct poses (factor 2)"),
    ("both_fixed", "both poses are fixed (factor 3)"),
    ("Z_nan", "Z is not finite (factor 1)"),
    ("Om_inf", "Omega is not finite (factor 4)"),
    ("T_nan", "T_jw is not finite (pose 3)"),
    ("unnamed", "pose 4 is optimisable but no factor names it"),
    ("no_pose", "n_pose must be >= 1"),
    ("no_factor", "n_rel must be >= 1: a pose graph needs a factor"),
    ("null_Z", "null factor array (factor 0)"),
    ("null_T", "null pose array"),
])
def test_refusals_name_the_factor_or_the_pose(built, create, what, where):
    T, fx, j, k, Z, Om = _good()
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
    elif what == "Om_inf":
        Om[4, 0, 5] = np.inf
    elif what == "T_nan":
        T[3, 4] = np.nan
    elif what == "unnamed":
        j[2], k[2] = 2, 3   # factors 2 and 4 become (2, 3) and (3, 2): nobody names pose 4
        j[4], k[4] = 3, 2
    elif what == "no_pose":
        kw["n_pose"] = 0
    elif what == "no_factor":
        kw["n_rel"] = 0
    elif what == "null_Z":
        Z = None
    elif what == "null_T":
        T, kw["n_pose"] = None, 5
    rc, msg = _call(create, T, fx, j, k, Z, Om, **kw)
    assert rc == -1 and msg == "ba_pgraph_create: " + where, msg


def test_python_wrapper_refuses_without_a_device(built):
    T, fx, j, k, Z, Om = _good()
    j[2], k[2] = 2, 3
    j[4], k[4] = 3, 2
    with pytest.raises(_lib.BaError, match="pose 4 is optimisable but no factor names it"):
        pgraph_check(T, fx, dict(j=j, k=k, Z=Z, Omega=Om))
