"""The C++ facade's FullBundleAdjustmentSolver::SolveBatch (cpp/tests/test_full_batch.cpp):
three windows through one batched launch against one Solve per solver object."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_solve_batch_is_declared_and_hooked_into_the_makefile():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    assert "static bool SolveBatch(const std::vector<FullBundleAdjustmentSolver *> &solvers" in hdr
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_full_batch:" in mk and "build/test_full_batch\n" in mk


@pytest.mark.gpu
def test_cpp_solve_batch_matches_single_solves_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_full_batch")
    assert os.path.exists(exe), "cpp/build/test_full_batch is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "FULL BATCH FACADE TEST PASSED" in r.stdout, r.stdout
