"""The C++ facade's FullBundleAdjustmentSolver::ComputeCovarianceBatch
(cpp/tests/test_batch_covariance.cpp): the blocks of three windows from one launch against
ComputeCovariance on each solver's own handle, zero blocks of fixed members, the refusal of
a sharded solver, the refactored class."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_compute_covariance_batch_is_declared_and_hooked_into_the_makefile():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    assert "static bool ComputeCovarianceBatch(const std::vector<FullBundleAdjustmentSolver *> &solvers, double sigma_pixel," in hdr
    assert "std::vector<std::vector<Eigen::Matrix<double, 6, 6>>> *cov_poses" in hdr
    assert "std::vector<std::vector<Eigen::Matrix<double, 3, 3>>> *cov_points" in hdr
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    assert "FullBundleAdjustmentSolver::ComputeCovarianceBatch(impls, sigma_pixel, cov_poses, cov_points)" in ref
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_batch_covariance:" in mk and "all: build/test_batch_covariance\n" in mk


@pytest.mark.gpu
def test_cpp_compute_covariance_batch_matches_the_handle_path_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_batch_covariance")
    assert os.path.exists(exe), "cpp/build/test_batch_covariance is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "BATCH COVARIANCE FACADE TEST PASSED" in r.stdout, r.stdout
