"""Host tests of the robust kernels of the pose-graph optimisation (no GPU): the new symbols and
their ctypes signatures, the kernel table, every refusal of ba_pgraph_robust_check, the calls on
a null object, and the refusals of the BA paths: set_relative (handle and batch), SolveBatch and
the full-BA Solve take no factor that carries a kernel."""
import ctypes as C

import numpy as np
import pytest

from bundle_adjustment_solver_amd import _lib
from bundle_adjustment_solver_amd.solver import (ROBUST_CAUCHY, ROBUST_GEMAN_MCCLURE, ROBUST_HUBER, ROBUST_NONE, SCALER,
                                                 BaBatch, BaProblem, FullBundleAdjustmentSolver,
                                                 FullBundleAdjustmentSolverRefactor, Options, pgraph_robust_check,
                                                 refuse_robust)


def test_symbols_and_signatures(built):
    lib = _lib.load()
    P, I32, D = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)
    want = {
        "ba_pgraph_set_robust": [P, I32, D],
        "ba_pgraph_robust_check": [C.c_int64, I32, D],
        "ba_pgraph_factor_report": [P, D, D],
    }
    for name, args in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    # null object: refused on the host, nothing touches a device
    assert lib.ba_pgraph_set_robust(None, None, None) == -1
    assert lib.ba_last_error().decode() == "ba_pgraph_set_robust: null graph"
    assert lib.ba_pgraph_factor_report(None, None, None) == -1
    names = [lib.ba_kernel_name(k).decode() for k in range(lib.ba_kernel_count())]
    assert "k_pg_lin_robust" in names and "k_pg_assemble_robust" in names
    assert len(set(names)) == len(names)
    assert (ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY, ROBUST_GEMAN_MCCLURE) == (0, 1, 2, 3)


def _check(kind, scale, n=None):
    lib = _lib.load()
    kd = None if kind is None else np.ascontiguousarray(kind, np.int32)
    sc = None if scale is None else np.ascontiguousarray(scale, np.float64)
    n = (0 if kd is None else len(kd)) if n is None else n
    rc = lib.ba_pgraph_robust_check(n, None if kd is None else kd.ctypes.data_as(C.POINTER(C.c_int32)),
                                    None if sc is None else sc.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, (lib.ba_last_error() or b"").decode()


def test_accepts(built):
    assert _check([0, 1, 2, 3], [0.0, 1.0, 30.0, 1e30])[0] == 0
    assert _check(None, None, 7)[0] == 0                      # NULL kinds clear every kernel
    assert _check([0, 0, 0], None)[0] == 0                    # all kinds 0: the scales are not read
    # the scale of a kind-0 factor is ignored, whatever it holds
    assert _check([0, 2, 0, 0], [np.nan, 1.0, -5.0, np.inf])[0] == 0
    assert _check([1], [np.nextafter(0.0, 1.0)])[0] == 0      # the smallest positive scale
    pgraph_robust_check([0, 3], [0.0, 2.0])


@pytest.mark.parametrize("kind,scale,where", [
    ([0, 4, 1], [1.0, 1.0, 1.0], "kind = 4 is not one of 0..3 (factor 1)"),
    ([-1], [1.0], "kind = -1 is not one of 0..3 (factor 0)"),
    ([1, 2, 3], [1.0, 1.0, 0.0], "scale must be > 0 (factor 2)"),
    ([1, 2, 3], [1.0, -3.0, 1.0], "scale must be > 0 (factor 1)"),
    ([3, 0, 0], [np.nan, 1.0, 1.0], "scale is not finite (factor 0)"),
    ([0, 0, 2], [1.0, 1.0, np.inf], "scale is not finite (factor 2)"),
    ([0, 0, 1], [1.0, 1.0, -np.inf], "scale is not finite (factor 2)"),
    ([0, 2], None, "null scale array (factor 1)"),
])
def test_refusals_name_the_factor(built, kind, scale, where):
    rc, msg = _check(kind, scale)
    assert rc == -1 and msg == "ba_pgraph_set_robust: " + where, msg
    if scale is not None:   # the Python wrapper raises with the same words
        with pytest.raises(_lib.BaError) as e:
            pgraph_robust_check(kind, scale)
        assert where in str(e.value)


def test_negative_count_is_refused(built):
    rc, msg = _check([1], [1.0], n=-1)
    assert rc == -1 and msg == "ba_pgraph_set_robust: n_rel must be >= 0"


# ---- the BA paths refuse a factor that carries a kernel ------------------------------------------
def _rels(kind):
    eye = np.r_[np.eye(3).reshape(9), np.zeros(3)]
    return dict(j=np.array([1, 2], np.int32), k=np.array([0, 1], np.int32), Z=np.tile(eye, (2, 1)),
                Omega=np.tile(np.eye(6), (2, 1, 1)), robust_kind=np.array(kind, np.int32),
                robust_scale=np.array([1.0, 1.0]))


def test_set_relative_refuses_robust_factors(built):
    # the refusal comes before the object is looked at: no handle, no device
    with pytest.raises(_lib.BaError, match=r"set_relative: factor 1 carries a robust kernel.*pose-graph only"):
        BaProblem.set_relative(None, _rels([0, 2]))
    with pytest.raises(_lib.BaError, match=r"set_relative: problem 1: factor 0 carries a robust kernel.*pose-graph only"):
        BaBatch.set_relative(type("B", (), dict(B=2))(), [None, _rels([3, 0])])
    refuse_robust("x", _rels([0, 0]))   # kinds that are all 0 carry no kernel
    refuse_robust("x", None)


@pytest.mark.parametrize("cls", [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor])
def test_facade_refuses_robust_factors_on_the_ba_paths(built, cls):
    s = cls(0)
    poses = np.tile(np.eye(4), (3, 1, 1))
    poses[:, 0, 3] = np.arange(3)
    hp = s.AddPoseArray(poses)
    s.MakePoseFixed(int(hp[0]))
    M = np.eye(4)
    M[0, 3] = 1.0
    s.AddRelativePose(int(hp[0]), int(hp[1]), M, np.eye(6))
    s.AddRelativePose(int(hp[1]), int(hp[2]), M, np.eye(6), sigma_pixel=0.5, robust=(ROBUST_CAUCHY, 3.0))
    rels = s._relative_arrays()
    assert rels["robust_kind"].tolist() == [0, 2]
    assert rels["robust_scale"].tolist() == [0.0, 3.0 * 0.5 * SCALER]   # times sigma_pixel SCALER
    with pytest.raises(_lib.BaError, match="factor 1 carries a robust kernel; robust factors are pose-graph only"):
        s.Solve(Options())
    assert s.is_parameter_finalized_ is False and s._problem is None
    with pytest.raises(_lib.BaError, match="factor 1 carries a robust kernel; robust factors are pose-graph only"):
        s.FinalizeParameters()
    fac = dict(pose_j=int(hp[1]), pose_k=int(hp[2]), measurement=M, information=np.eye(6), robust=(ROBUST_HUBER, 1.0))
    for what in ("SolveBatch", "ComputeCovarianceBatch", "MarginalizeBatch"):
        with pytest.raises(_lib.BaError, match="%s: factor 0 carries a robust kernel; robust factors are pose-graph only"
                           % what):
            cls._scaled_relatives(what, [s], [[fac]], 1.0)
    # a kernel that the check refuses is refused when the factor is added
    with pytest.raises(_lib.BaError, match="scale must be > 0"):
        s.AddRelativePose(int(hp[1]), int(hp[2]), M, np.eye(6), robust=(ROBUST_GEMAN_MCCLURE, 0.0))
    with pytest.raises(_lib.BaError, match="kind = 7"):
        s.AddRelativePose(int(hp[1]), int(hp[2]), M, np.eye(6), robust=(7, 1.0))
    assert len(s._relatives) == 2
    # robust=None and kind 0 are the factor of before
    t = cls(0)
    hq = t.AddPoseArray(poses.copy())
    t.AddRelativePose(int(hq[0]), int(hq[1]), M, np.eye(6), robust=(ROBUST_NONE, 0.0))
    assert sorted(t._relative_arrays()) == ["Omega", "Z", "j", "k"]
