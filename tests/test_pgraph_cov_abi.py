"""Host tests of the pose graph's covariance and gate (no GPU): the new symbols and their ctypes
signatures, the calls on a null object, every refusal of ba_pgraph_cov_check with its message,
the kernel table, and the facades' refusal of factors given with different sigma_pixel."""
import ctypes as C

import numpy as np
import pytest

from bundle_adjustment_solver_amd import _lib
from bundle_adjustment_solver_amd.solver import (FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor,
                                                 pgraph_cov_check)

I32, D, I64, U8 = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)


def test_symbols_and_signatures(built):
    lib = _lib.load()
    P = C.c_void_p
    want = {
        "ba_pgraph_covariance": [P, C.c_int, I32, D, C.c_int64, I32, I32, D, D, I64],
        "ba_pgraph_gate": [P, C.c_int64, I32, I32, D, D, D, D, D, I64],
        "ba_pgraph_cov_check": [C.c_int, U8, C.c_int, I32, D, C.c_int64, I32, I32, D, C.c_int64, I32, I32, D, D, D],
        "ba_pgraph_cov_info": [P, I64],
    }
    for name, args in want.items():
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == args, name
    # null object: refused on the host, nothing touches a device
    assert lib.ba_pgraph_covariance(None, 0, None, None, 0, None, None, None, None, None) == -1
    assert lib.ba_last_error().decode() == "ba_pgraph_covariance: null graph"
    assert lib.ba_pgraph_gate(None, 0, None, None, None, None, None, None, None, None) == -1
    assert lib.ba_last_error().decode() == "ba_pgraph_gate: null graph"
    assert lib.ba_pgraph_cov_info(None, (C.c_int64 * 4)()) == -1


def test_the_kernel_table_is_unchanged(built):
    """the new kernels run outside the iteration: not in the table, not timed"""
    lib = _lib.load()
    names = [lib.ba_kernel_name(k).decode() for k in range(lib.ba_kernel_count())]
    assert not [n for n in names if "pgcov" in n or "cov" in n]


FIXED = np.array([1, 0, 0, 1, 0], np.uint8)   # five poses, 0 and 3 fixed
EYE = np.r_[np.eye(3).reshape(9), np.zeros(3)]


def _check(sel=None, pairs=None, cands=None, out_pose=True, out_rel=True, out_d2=True, fixed=FIXED, n_pose=5):
    lib = _lib.load()
    keep = []

    def arr(a, dt, ptr):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data_as(ptr)
    out = np.zeros(36 * 8)
    o = out.ctypes.data_as(D)
    sel = [] if sel is None else sel
    pj, pk = ([], []) if pairs is None else pairs
    cj, ck, Z, Om = ([], [], None, None) if cands is None else cands
    rc = lib.ba_pgraph_cov_check(n_pose, arr(fixed, np.uint8, U8), len(sel), arr(sel, np.int32, I32),
                                 o if out_pose else None, len(pj), arr(pj, np.int32, I32), arr(pk, np.int32, I32),
                                 o if out_rel else None, len(cj), arr(cj, np.int32, I32), arr(ck, np.int32, I32),
                                 arr(Z, np.float64, D), arr(Om, np.float64, D), o if out_d2 else None)
    return rc, (lib.ba_last_error() or b"").decode()


def _cand(j, k, Z=None, Om=None):
    n = len(j)
    return (j, k, np.tile(EYE, (n, 1)) if Z is None else Z, np.tile(np.eye(6), (n, 1, 1)) if Om is None else Om)


def test_accepts(built):
    assert _check()[0] == 0                                              # nothing selected
    assert _check(sel=[4, 1, 1, 2], pairs=([1, 0, 2, 2], [2, 1, 1, 1]))[0] == 0   # repeats, both ways, j fixed
    assert _check(sel=[1], pairs=([1], [3]), fixed=None)[0] == 0       # no mask: none fixed
    assert _check(cands=_cand([4, 0], [1, 4]))[0] == 0
    # only the lower triangle of Omega counts: garbage above the diagonal is not read
    Om = np.tile(np.eye(6), (1, 1, 1))
    Om[0, 0, 5] = -1e9
    assert _check(cands=_cand([1], [2], Om=Om))[0] == 0
    assert _check(out_pose=False, out_rel=False, out_d2=False)[0] == 0   # NULL outputs of empty selections
    pgraph_cov_check(5, FIXED, [1, 2], ([1], [2]), dict(j=[4], k=[0], Z=EYE, Omega=np.eye(6)))


def _nonfinite(what):
    Z, Om = np.tile(EYE, (2, 1)), np.tile(np.eye(6), (2, 1, 1))
    (Z if what == "Z" else Om).reshape(2, -1)[1, 3] = np.nan
    return _cand([1, 2], [2, 4], Z, Om)


def _not_spd(kind):
    Om = np.tile(np.eye(6), (3, 1, 1))
    if kind == "indefinite":
        Om[2, 4, 4] = -1.0
    elif kind == "singular":
        Om[2] = np.ones((6, 6))
    else:   # only the LOWER triangle counts: a lower triangle that is not positive definite
        Om[2, 3, 1] = 5.0
    return _cand([1, 2, 4], [2, 4, 1], Om=Om)


@pytest.mark.parametrize("kw,msg", [
    (dict(sel=[1], out_pose=False), "ba_pgraph_covariance: cov_pose36 is NULL for a non-empty pose selection"),
    (dict(pairs=([1], [2]), out_rel=False), "ba_pgraph_covariance: cov_rel36 is NULL for a non-empty pair selection"),
    (dict(cands=_cand([1], [2]), out_d2=False), "ba_pgraph_gate: d2 is NULL for a non-empty candidate list"),
    (dict(sel=[1, 5]), "ba_pgraph_covariance: pose_sel[1] = 5 is out of range"),
    (dict(sel=[-1]), "ba_pgraph_covariance: pose_sel[0] = -1 is out of range"),
    (dict(sel=[1, 2, 3]), "ba_pgraph_covariance: pose_sel[2] = 3 is a fixed pose"),
    (dict(pairs=([1, 7], [2, 1])), "ba_pgraph_covariance: pose j = 7 out of range (pair 1)"),
    (dict(pairs=([1], [-2])), "ba_pgraph_covariance: pose k = -2 out of range (pair 0)"),
    (dict(pairs=([1, 2, 4], [2, 4, 4])), "ba_pgraph_covariance: j == k: a factor needs two distinct poses (pair 2)"),
    (dict(pairs=([1, 0], [2, 3])), "ba_pgraph_covariance: both poses are fixed (pair 1)"),
    (dict(cands=_cand([1, 9], [2, 1])), "ba_pgraph_gate: pose j = 9 out of range (candidate 1)"),
    (dict(cands=_cand([1], [5])), "ba_pgraph_gate: pose k = 5 out of range (candidate 0)"),
    (dict(cands=_cand([2], [2])), "ba_pgraph_gate: j == k: a factor needs two distinct poses (candidate 0)"),
    (dict(cands=_cand([1, 3], [2, 0])), "ba_pgraph_gate: both poses are fixed (candidate 1)"),
    (dict(cands=_nonfinite("Z")), "ba_pgraph_gate: Z is not finite (candidate 1)"),
    (dict(cands=_nonfinite("Omega")), "ba_pgraph_gate: Omega is not finite (candidate 1)"),
    (dict(cands=_not_spd("indefinite")), "ba_pgraph_gate: Omega is not positive definite (candidate 2)"),
    (dict(cands=_not_spd("singular")), "ba_pgraph_gate: Omega is not positive definite (candidate 2)"),
    (dict(cands=_not_spd("lower")), "ba_pgraph_gate: Omega is not positive definite (candidate 2)"),
    (dict(n_pose=0, fixed=None), "ba_pgraph_covariance: n_pose must be >= 1"),
])
def test_refusals_name_the_entry(built, kw, msg):
    rc, got = _check(**kw)
    assert rc == -1 and got == msg, got


def test_the_python_wrapper_raises_with_the_same_words(built):
    with pytest.raises(_lib.BaError, match=r"pose_sel\[0\] = 0 is a fixed pose"):
        pgraph_cov_check(5, FIXED, [0])
    with pytest.raises(_lib.BaError, match=r"both poses are fixed \(pair 0\)"):
        pgraph_cov_check(5, FIXED, pairs=[(0, 3)])
    with pytest.raises(_lib.BaError, match=r"Omega is not positive definite \(candidate 0\)"):
        pgraph_cov_check(5, FIXED, candidates=dict(j=[1], k=[2], Z=EYE, Omega=-np.eye(6)))


@pytest.mark.parametrize("cls", [FullBundleAdjustmentSolver, FullBundleAdjustmentSolverRefactor])
def test_facade_refuses_mixed_sigma_pixel(built, cls):
    """Sigma and d2 have caller's units only for one sigma_pixel; refused before any device work"""
    s = cls(0)
    poses = np.tile(np.eye(4), (3, 1, 1))
    poses[:, 0, 3] = np.arange(3)
    hp = s.AddPoseArray(poses)
    s.MakePoseFixed(int(hp[0]))
    M = np.eye(4)
    M[0, 3] = 1.0
    s.AddRelativePose(int(hp[0]), int(hp[1]), M, np.eye(6), sigma_pixel=2.0)
    cand = dict(pose_j=int(hp[2]), pose_k=int(hp[0]), measurement=M, information=np.eye(6))
    with pytest.raises(RuntimeError, match=r"GateLoopClosures: .*sigma_pixel = 2 and 1"):
        s.GateLoopClosures([cand])
    s.AddRelativePose(int(hp[1]), int(hp[2]), M, np.eye(6), sigma_pixel=0.5)
    with pytest.raises(RuntimeError, match=r"ComputePoseGraphCovariance: .*sigma_pixel = 2 and 0.5"):
        s.ComputePoseGraphCovariance([int(hp[1])])
    with pytest.raises(RuntimeError, match=r"GateLoopClosures: .*sigma_pixel = 2 and 0.5"):
        s.GateLoopClosures([dict(cand, sigma_pixel=2.0)])
    t = cls(0)
    t.AddPoseArray(poses.copy())
    with pytest.raises(RuntimeError, match="ComputePoseGraphCovariance: poses .* must be added first"):
        t.ComputePoseGraphCovariance([0])
