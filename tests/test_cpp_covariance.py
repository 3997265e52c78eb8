"""The C++ facade's FullBundleAdjustmentSolver::ComputeCovariance
(cpp/tests/test_covariance.cpp): the facade's blocks against ba_covariance on the same
handle after the unit conversion, the refusals, the refactored class."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_compute_covariance_is_declared_and_hooked_into_the_makefile():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    assert "bool ComputeCovariance(const std::vector<_BA_Pose *> &poses, const std::vector<_BA_Point *> &points," in hdr
    assert "std::vector<Eigen::Matrix<double, 6, 6>> *cov_poses" in hdr
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    assert "impl_.ComputeCovariance(poses, points, sigma_pixel, cov_poses, cov_points)" in ref
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_covariance:" in mk and "build/test_covariance\n" in mk


@pytest.mark.gpu
def test_cpp_compute_covariance_matches_the_c_abi_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_covariance")
    assert os.path.exists(exe), "cpp/build/test_covariance is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "COVARIANCE FACADE TEST PASSED" in r.stdout, r.stdout
