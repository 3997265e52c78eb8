"""The C++ facades' relative-pose factors of a solver's own problem (cpp/tests/test_relative.cpp):
AddRelativePose of FullBundleAdjustmentSolver and FullBundleAdjustmentSolverRefactor in the
caller's units against ba_set_relative + ba_solve called directly through include/ba_hip.h in
scaled units, to the bit; an unknown pose throws; after FinalizeParameters the call is ignored;
ReloadParameterValues keeps the factors and Reset drops them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_add_relative_pose_is_declared_and_hooked_into_the_makefile():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    assert "void AddRelativePose(const RelativePose &factor, double sigma_pixel = 1.0);" in hdr
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    assert "void AddRelativePose(const RelativePose &factor, double sigma_pixel = 1.0) {" in ref
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_relative:" in mk and "all: build/test_relative\n" in mk
    abi = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("int ba_set_relative(ba_handle *h", "int ba_update_relative(ba_handle *h", "int ba_relative_check(",
                 "int ba_relative_info(ba_handle *h"):
        assert name in abi, name


@pytest.mark.gpu
def test_cpp_add_relative_pose_matches_the_direct_call_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_relative")
    assert os.path.exists(exe), "cpp/build/test_relative is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "RELATIVE FACADE TEST PASSED" in r.stdout, r.stdout
