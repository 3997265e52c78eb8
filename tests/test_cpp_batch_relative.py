"""The C++ facades' relative-pose factors (cpp/tests/test_batch_relative.cpp): SolveBatch with
in_relatives in the caller's units against ba_batch_set_relative + ba_batch_solve called directly
through include/ba_hip.h in scaled units, to the bit; the chain SolveBatch -> MarginalizeBatch ->
SolveBatch on both classes; the refusals."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_relative_pose_is_declared_and_hooked_into_the_makefile():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    assert "struct RelativePose {" in hdr
    assert hdr.count("const std::vector<std::vector<RelativePose>> *in_relatives = nullptr") == 3
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    assert "using RelativePose = FullBundleAdjustmentSolver::RelativePose;" in ref
    assert ref.count("const std::vector<std::vector<RelativePose>> *in_relatives") == 3
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_batch_relative:" in mk and "all: build/test_batch_relative\n" in mk


@pytest.mark.gpu
def test_cpp_batch_calls_with_relatives_match_the_direct_call_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_batch_relative")
    assert os.path.exists(exe), "cpp/build/test_batch_relative is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "BATCH RELATIVE FACADE TEST PASSED" in r.stdout, r.stdout
