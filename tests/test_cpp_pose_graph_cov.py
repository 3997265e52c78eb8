"""The pose graph's covariance and gate on the C++ facades (cpp/tests/test_pose_graph_cov.cpp):
ComputePoseGraphCovariance and GateLoopClosures of FullBundleAdjustmentSolver and
FullBundleAdjustmentSolverRefactor against ba_pgraph_covariance + ba_pgraph_gate called directly,
converted by the unit relations of the header (1e-12 relative); a true candidate passes the gate,
a false one does not; factors with two values of sigma_pixel are refused."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_covariance_surface_is_declared_and_hooked_into_the_makefiles():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    assert "bool ComputePoseGraphCovariance(const std::vector<_BA_Pose *> &poses," in hdr
    assert "bool GateLoopClosures(const std::vector<RelativePose> &candidates, double sigma_pixel," in hdr
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    assert "bool ComputePoseGraphCovariance(" in ref and "bool GateLoopClosures(" in ref
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_pose_graph_cov:" in mk and "all: build/test_pose_graph_cov\n" in mk
    abi = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("int ba_pgraph_covariance(ba_pgraph *g", "int ba_pgraph_gate(ba_pgraph *g",
                 "int ba_pgraph_cov_check(int n_pose", "int ba_pgraph_cov_info(ba_pgraph *g"):
        assert name in abi, name
    lib_mk = open(os.path.join(ROOT, "bundle_adjustment_solver_amd", "csrc", "Makefile")).read()
    assert "ba_graph_kernels.o" in lib_mk and "dbg/ba_graph_kernels.o" in lib_mk


@pytest.mark.gpu
def test_cpp_pose_graph_covariance_matches_the_direct_call_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_pose_graph_cov")
    assert os.path.exists(exe), "cpp/build/test_pose_graph_cov is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "POSE GRAPH COVARIANCE FACADE TEST PASSED" in r.stdout, r.stdout
