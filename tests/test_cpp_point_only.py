"""The C++ facades' structure-only solve (cpp/tests/test_point_only.cpp): SolvePointsOnly of
FullBundleAdjustmentSolver and FullBundleAdjustmentSolverRefactor in the caller's units
against ba_point_only called directly through include/ba_hip.h in scaled units, to the bit;
fixed points and every pose untouched; a NaN point triangulated; a Solve on the same object
afterwards; the refusals."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_solve_points_only_is_declared_and_hooked_into_the_makefile():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    assert "struct PointOnlyResult {" in hdr
    assert "bool SolvePointsOnly(Options options, std::vector<PointOnlyResult> *results = nullptr," in hdr
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    assert "using PointOnlyResult = FullBundleAdjustmentSolver::PointOnlyResult;" in ref
    assert "bool SolvePointsOnly(Options options, std::vector<PointOnlyResult> *results = nullptr," in ref
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_point_only:" in mk and "all: build/test_point_only\n" in mk
    abi = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    assert "int ba_point_only(ba_handle *h" in abi and "int ba_point_only_check(" in abi


@pytest.mark.gpu
def test_cpp_solve_points_only_matches_the_direct_call_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_point_only")
    assert os.path.exists(exe), "cpp/build/test_point_only is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "POINT ONLY FACADE TEST PASSED" in r.stdout, r.stdout
