"""ba_batch_covariance: the parts that need no GPU — declaration, export, binding, the
result record, the NULL checks that run before anything touches a device, and the Python
entry points (a sharded solver is refused before any array is built)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bundle_adjustment_solver_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ba_batch_covariance"


def test_symbol_declared_exported_bound(built):
    src = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    lib = _lib.load()
    m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % NAME, src, re.S)
    assert m, "not declared in ba_hip.h"
    assert hasattr(lib, NAME), "missing export"
    assert NAME in _lib.SIGNATURES
    n_decl = len([a for a in m.group(1).split(",") if a.strip()])
    assert n_decl == len(_lib.SIGNATURES[NAME][1]) == 5


def test_result_record_is_two_ints(built):
    src = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    m = re.search(r"typedef struct \{\s*int ([^;]*);\s*\}\s*ba_batch_cov_result;", src, re.S)
    assert m
    assert [f.strip() for f in m.group(1).split(",")] == ["status", "dropped_pivots"]
    assert _lib.BaBatchCovResult._fields_ == [("status", C.c_int), ("dropped_pivots", C.c_int)]
    assert C.sizeof(_lib.BaBatchCovResult) == 8


def test_null_arguments_are_refused_without_a_gpu(built):
    """The batch pointer is looked at first: no batch exists in this test (there is no GPU
    to create one on), so only that check can be driven here."""
    lib = _lib.load()
    cp = np.zeros(36)
    res = (_lib.BaBatchCovResult * 1)()
    rc = lib.ba_batch_covariance(None, 1.0, cp.ctypes.data_as(C.POINTER(C.c_double)), None, res)
    assert rc == -1
    err = lib.ba_last_error().decode()
    assert NAME in err and "null batch" in err
    assert lib.ba_batch_covariance(None, 1.0, None, None, None) == -1


def test_python_entry_points_exist():
    from bundle_adjustment_solver_amd.solver import BaBatch, FullBundleAdjustmentSolver
    for name in ("covariance", "cov_poses_of", "cov_points_of"):
        assert callable(getattr(BaBatch, name))
    assert callable(FullBundleAdjustmentSolver.ComputeCovarianceBatch)
    assert FullBundleAdjustmentSolver.ComputeCovarianceBatch([]) == []


def test_python_covariance_batch_refuses_a_sharded_solver():
    """As SolveBatch: a solver with a shard or an all-reduce configured cannot join a batch;
    refused before any array is built or a device is touched."""
    from bundle_adjustment_solver_amd.solver import FullBundleAdjustmentSolver
    plain, sharded, hooked = (FullBundleAdjustmentSolver(0) for _ in range(3))
    sharded.SetShard(0, 2)
    hooked.SetShard(0, 1, allreduce=lambda which, ptr, n, stream: 0)
    for bad in (sharded, hooked):
        with pytest.raises(RuntimeError, match="shard or an all-reduce"):
            FullBundleAdjustmentSolver.ComputeCovarianceBatch([plain, bad])
