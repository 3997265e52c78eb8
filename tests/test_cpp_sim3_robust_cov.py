"""The C++ facades' robust kernels, covariance blocks and gate of the Sim(3) graph
(cpp/tests/test_sim3_robust_cov.cpp): RelativeSim3::robust_kind / robust_scale, SolveSim3Graph,
GetRelativeSim3Weights, ComputeSim3GraphCovariance and GateSim3LoopClosures of
FullBundleAdjustmentSolver and FullBundleAdjustmentSolverRefactor in the caller's units against
ba_sim3_* called directly through include/ba_hip.h in scaled units, to the bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_the_calls_are_declared_and_hooked_into_the_makefiles():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    for text in (hdr, ref):
        assert "void GetRelativeSim3Weights(std::vector<double> *s, std::vector<double> *w) const" in text
        assert "bool ComputeSim3GraphCovariance(" in text and "std::vector<Eigen::Matrix<double, 7, 7>> *cov_rel" in text
        assert "bool GateSim3LoopClosures(const std::vector<RelativeSim3> &candidates, double sigma_pixel, " \
               "std::vector<double> *d2)" in text
    assert "int robust_kind{0};" in hdr.split("struct RelativeSim3 {")[1].split("\n  };")[0]
    assert "double robust_scale{0.0};" in hdr.split("struct RelativeSim3 {")[1].split("\n  };")[0]
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_sim3_robust_cov:" in mk and "all: build/test_sim3_robust_cov\n" in mk
    lib_mk = open(os.path.join(ROOT, "bundle_adjustment_solver_amd", "csrc", "Makefile")).read()
    assert "ba_graph_kernels.o" in lib_mk and "ba_robust_fn.h" in lib_mk
    abi = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("int ba_sim3_set_robust(ba_sim3 *g", "int ba_sim3_robust_check(int64_t n_rel",
                 "int ba_sim3_factor_weights(ba_sim3 *g", "int ba_sim3_covariance(ba_sim3 *g",
                 "int ba_sim3_gate(ba_sim3 *g", "int ba_sim3_cov_check(int n_pose", "int ba_sim3_cov_info(ba_sim3 *g",
                 "int ba_sim3_factor_report(ba_sim3 *g, double *s);"):
        assert name in abi, name


@pytest.mark.gpu
def test_cpp_sim3_robust_cov_matches_the_direct_calls_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_sim3_robust_cov")
    assert os.path.exists(exe), "cpp/build/test_sim3_robust_cov is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "SIM3 ROBUST COV FACADE TEST PASSED" in r.stdout, r.stdout
