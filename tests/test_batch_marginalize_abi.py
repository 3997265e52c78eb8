"""ba_batch_marginalize: the parts that need no GPU — declaration, export, binding, the
result record, the host-only plan of one problem against a numpy restatement, the unit
conversion, the NULL checks that run before anything touches a device, and the Python
entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bundle_adjustment_solver_amd import _lib
from bundle_adjustment_solver_amd.solver import covariance_to_user_units, marginal_to_user_units

import marg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"ba_batch_marginalize": 7, "ba_batch_marg_layout": 4, "ba_batch_marg_plan_problem": 10}


def test_symbols_declared_exported_bound(built):
    src = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    lib = _lib.load()
    for name, n_arg in NAMES.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, src, re.S)
        assert m, "%s not declared in ba_hip.h" % name
        assert hasattr(lib, name), "missing export"
        n_decl = len([a for a in m.group(1).split(",") if a.strip()])
        assert n_decl == len(_lib.SIGNATURES[name][1]) == n_arg


def test_result_record_is_five_ints(built):
    src = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    m = re.search(r"typedef struct \{\s*int ([^;]*);\s*\}\s*ba_batch_marg_result;", src, re.S)
    assert m
    fields = ["status", "dropped_pivots", "n_kept", "n_marg_pose", "n_marg_pt"]
    assert [f.strip() for f in m.group(1).split(",")] == fields
    assert _lib.BaBatchMargResult._fields_ == [(f, C.c_int) for f in fields]
    assert C.sizeof(_lib.BaBatchMargResult) == 20


def _plan(pose_fixed, marg, pt_fixed, obs_pose, obs_pt, kept=True, mq=True, n_pt=None):
    lib = _lib.load()
    n_pose, n_pt = len(marg), len(pt_fixed) if n_pt is None else n_pt
    k = np.full(max(1, n_pose), -7, np.int32)
    q = np.full(max(1, n_pt), 9, np.uint8)
    u8 = lambda a: None if a is None else np.ascontiguousarray(a, np.uint8).ctypes.data_as(_lib._U8)
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(_lib._I32)
    K = lib.ba_batch_marg_plan_problem(n_pose, u8(pose_fixed), u8(marg), n_pt, u8(pt_fixed),
                                       0 if obs_pose is None else len(obs_pose), i32(obs_pose), i32(obs_pt),
                                       k.ctypes.data_as(_lib._I32) if kept else None,
                                       q.ctypes.data_as(_lib._U8) if mq else None)
    return K, k, q[:n_pt]


def test_plan_problem_matches_the_numpy_restatement(built):
    rng = np.random.default_rng(5)
    seen_fixed_marked = seen_unobserved = seen_fixed_pt = False
    for trial in range(40):
        n_pose, n_pt = int(rng.integers(1, 9)), int(rng.integers(1, 14))
        n_obs = int(rng.integers(0, 40))
        pr = dict(pose_fixed=(rng.random(n_pose) < 0.3).astype(np.uint8),
                  pt_fixed=(rng.random(n_pt) < 0.25).astype(np.uint8),
                  obs_pose=rng.integers(0, n_pose, n_obs).astype(np.int32),
                  obs_pt=rng.integers(0, max(1, n_pt - 2), n_obs).astype(np.int32))  # the last points: unobserved
        mk = (rng.random(n_pose) < 0.4).astype(np.uint8)
        kept, in_l = marg_ref.plan(pr, mk)
        K, k, q = _plan(pr["pose_fixed"], mk, pr["pt_fixed"], pr["obs_pose"], pr["obs_pt"])
        assert K == len(kept) and np.array_equal(k[:K], kept) and (k[K:] == -7).all()
        assert (np.diff(k[:K]) > 0).all()
        assert np.array_equal(q != 0, in_l) and set(q) <= {0, 1}
        assert not (q[pr["pt_fixed"] != 0]).any()                          # fixed points never in L
        assert not q[np.bincount(pr["obs_pt"], minlength=n_pt) == 0].any()  # unobserved points never in L
        by_fixed = np.zeros(n_pt, bool)
        by_fixed[pr["obs_pt"][(mk[pr["obs_pose"]] != 0) & (pr["pose_fixed"][pr["obs_pose"]] != 0)]] = True
        seen_fixed_marked |= bool((by_fixed & (q != 0)).any())     # a marked FIXED pose selects landmarks
        seen_unobserved |= n_pt >= 3
        seen_fixed_pt |= bool(pr["pt_fixed"].any())
        # either output may be NULL; pose_fixed / pt_fixed NULL = none fixed
        assert _plan(pr["pose_fixed"], mk, pr["pt_fixed"], pr["obs_pose"], pr["obs_pt"], False, False)[0] == K
        K0, k0, q0 = _plan(None, mk, None, pr["obs_pose"], pr["obs_pt"], n_pt=n_pt)
        z = dict(pr, pose_fixed=np.zeros(n_pose, np.uint8), pt_fixed=np.zeros(n_pt, np.uint8))
        kz, lz = marg_ref.plan(z, mk)
        assert K0 == len(kz) and np.array_equal(k0[:K0], kz) and np.array_equal(q0 != 0, lz)
    assert seen_fixed_marked and seen_unobserved and seen_fixed_pt


def test_plan_problem_refuses_bad_input(built):
    lib = _lib.load()
    mk, pf, qf = np.zeros(3, np.uint8), np.zeros(3, np.uint8), np.zeros(4, np.uint8)
    ok = (np.array([0, 2], np.int32), np.array([1, 3], np.int32))
    assert _plan(pf, mk, qf, *ok)[0] == 3
    for op, oq in (([0, 3], [1, 3]), ([0, -1], [1, 3]), ([0, 2], [1, 4]), ([0, 2], [-1, 3])):
        assert _plan(pf, mk, qf, np.array(op, np.int32), np.array(oq, np.int32))[0] == -1
        assert "out of range" in lib.ba_last_error().decode()
    u8 = lambda a: a.ctypes.data_as(_lib._U8)
    i32 = lambda a: a.ctypes.data_as(_lib._I32)
    assert lib.ba_batch_marg_plan_problem(3, u8(pf), None, 4, u8(qf), 2, i32(ok[0]), i32(ok[1]), None, None) == -1
    assert "null marg_pose" in lib.ba_last_error().decode()
    assert lib.ba_batch_marg_plan_problem(3, u8(pf), u8(mk), 4, u8(qf), 2, None, i32(ok[1]), None, None) == -1
    assert lib.ba_batch_marg_plan_problem(3, u8(pf), u8(mk), 4, u8(qf), 2, i32(ok[0]), None, None, None) == -1
    assert "null observations" in lib.ba_last_error().decode()
    assert lib.ba_batch_marg_plan_problem(-1, u8(pf), u8(mk), 4, u8(qf), 0, None, None, None, None) == -1
    assert lib.ba_batch_marg_plan_problem(3, u8(pf), u8(mk), 4, u8(qf), -1, None, None, None, None) == -1


def test_user_units_invert_the_covariance_units():
    """H_u Cov_u == H_s Sigma_s: information and covariance of one Gaussian stay inverse to
    each other through the two conversions."""
    rng = np.random.default_rng(3)
    for K, sigma in ((1, 1.0), (3, 0.7), (5, 2.5)):
        G = rng.standard_normal((6 * K, 6 * K + 4))
        Hs = G @ G.T
        bs = rng.standard_normal(6 * K)
        Sig = np.linalg.inv(Hs)
        Hu, bu = marginal_to_user_units(Hs, bs, sigma)
        assert Hu.shape == Hs.shape and bu.shape == bs.shape and np.array_equal(Hu, Hu.T)
        # the covariance conversion works per 6x6 block: check block products on the diagonal
        blocks = np.stack([Sig[6 * j:6 * j + 6, 6 * j:6 * j + 6] for j in range(K)])
        cu, _ = covariance_to_user_units(blocks, np.zeros((0, 3, 3)), sigma)
        d = np.tile(np.r_[np.full(3, 100.0), np.ones(3)], K)
        Sig_u = (sigma ** 2 * 1e-4) * (d[:, None] * Sig * d[None, :])
        for j in range(K):
            assert np.allclose(Sig_u[6 * j:6 * j + 6, 6 * j:6 * j + 6], cu[j], rtol=1e-14, atol=0)
        assert np.allclose(Hu @ Sig_u, Hs @ Sig, rtol=0, atol=1e-9)
        assert np.allclose(Hu @ Sig_u, np.eye(6 * K), rtol=0, atol=1e-9)
        # the Gauss-Newton step is the same vector in the two unit systems
        assert np.allclose(np.linalg.solve(Hu, bu), d * np.linalg.solve(Hs, bs), rtol=1e-9)
    H0, b0 = marginal_to_user_units(np.zeros((0, 0)), np.zeros(0), 1.0)
    assert H0.shape == (0, 0) and b0.shape == (0,)


def test_null_arguments_are_refused_without_a_gpu(built):
    """The batch pointer is looked at first: no batch exists in this test (there is no GPU
    to create one on), so only that check can be driven here."""
    lib = _lib.load()
    H, b, mk = np.zeros(36), np.zeros(6), np.zeros(1, np.uint8)
    res = (_lib.BaBatchMargResult * 1)()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.ba_batch_marginalize(None, 1.0, mk.ctypes.data_as(_lib._U8), dp(H), dp(b), None, res)
    assert rc == -1
    err = lib.ba_last_error().decode()
    assert "ba_batch_marginalize" in err and "null batch" in err
    assert lib.ba_batch_marginalize(None, 1.0, None, None, None, None, None) == -1
    off = np.zeros(2, np.int64)
    i64 = off.ctypes.data_as(C.POINTER(C.c_int64))
    assert lib.ba_batch_marg_layout(None, mk.ctypes.data_as(_lib._U8), i64, i64) == -1
    assert "ba_batch_marg_layout" in lib.ba_last_error().decode()


def test_python_entry_points_exist():
    import bundle_adjustment_solver_amd as pkg
    from bundle_adjustment_solver_amd.solver import BaBatch, FullBundleAdjustmentSolver
    for name in ("marginalize", "marg_layout"):
        assert callable(getattr(BaBatch, name))
    assert pkg.marginal_to_user_units is marginal_to_user_units
    assert FullBundleAdjustmentSolver.MarginalizeBatch([], []) == []


def test_python_marginalize_batch_refuses_bad_arguments():
    from bundle_adjustment_solver_amd.solver import FullBundleAdjustmentSolver
    plain, sharded = FullBundleAdjustmentSolver(0), FullBundleAdjustmentSolver(0)
    sharded.SetShard(0, 2)
    with pytest.raises(RuntimeError, match="shard or an all-reduce"):
        FullBundleAdjustmentSolver.MarginalizeBatch([plain, sharded], [[], []])
    with pytest.raises(ValueError, match="one list of poses per solver"):
        FullBundleAdjustmentSolver.MarginalizeBatch([plain], [])
