"""The C++ facade's pose prior (cpp/tests/test_batch_prior.cpp): SolveBatch with in_priors in
the caller's units against ba_batch_set_prior + ba_batch_solve called directly through
include/ba_hip.h in scaled units, to the bit; the other two batch entry points, the refusals,
the refactored class."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_pose_prior_is_declared_and_hooked_into_the_makefile():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    assert "struct PosePrior {" in hdr
    assert hdr.count("const std::vector<PosePrior> *in_priors = nullptr") == 3
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    assert "MarginalizeBatch(impls, marg_poses, sigma_pixel, priors, in_priors)" in ref
    assert "ComputeCovarianceBatch(impls, sigma_pixel, cov_poses, cov_points, in_priors)" in ref
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_batch_prior:" in mk and "all: build/test_batch_prior\n" in mk


@pytest.mark.gpu
def test_cpp_solve_batch_with_priors_matches_the_direct_call_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_batch_prior")
    assert os.path.exists(exe), "cpp/build/test_batch_prior is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "BATCH PRIOR FACADE TEST PASSED" in r.stdout, r.stdout
