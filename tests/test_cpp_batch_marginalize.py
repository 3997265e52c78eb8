"""The C++ facade's FullBundleAdjustmentSolver::MarginalizeBatch
(cpp/tests/test_batch_marginalize.cpp): the priors of two windows from one launch against
ba_batch_marginalize called directly on the same arrays after the unit conversion, the kept
and marginalised pointer lists, the refusals, the refactored class."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_marginalize_batch_is_declared_and_hooked_into_the_makefile():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    assert "static bool MarginalizeBatch(const std::vector<FullBundleAdjustmentSolver *> &solvers," in hdr
    assert "const std::vector<std::vector<_BA_Pose *>> &marg_poses, double sigma_pixel," in hdr
    assert "struct MarginalPrior {" in hdr
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    assert "FullBundleAdjustmentSolver::MarginalizeBatch(impls, marg_poses, sigma_pixel, priors)" in ref
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_batch_marginalize:" in mk and "all: build/test_batch_marginalize\n" in mk


@pytest.mark.gpu
def test_cpp_marginalize_batch_matches_the_direct_call_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_batch_marginalize")
    assert os.path.exists(exe), "cpp/build/test_batch_marginalize is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "BATCH MARGINALIZE FACADE TEST PASSED" in r.stdout, r.stdout
