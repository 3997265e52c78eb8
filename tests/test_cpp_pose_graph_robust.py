"""Robust loop-closure factors on the C++ facades (cpp/tests/test_pose_graph_robust.cpp):
RelativePose::robust_kind / robust_scale through AddRelativePose, SolvePoseGraph and
GetRelativeWeights of FullBundleAdjustmentSolver and FullBundleAdjustmentSolverRefactor against
ba_pgraph_set_robust + ba_pgraph_solve + ba_pgraph_factor_report called directly, to the bit; the
false closure ends with a small weight; the BA paths refuse a factor that carries a kernel."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_robust_surface_is_declared_and_hooked_into_the_makefiles():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    assert "int robust_kind{0};" in hdr and "double robust_scale{0.0};" in hdr
    assert "void GetRelativeWeights(std::vector<double> *s, std::vector<double> *w) const;" in hdr
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    assert "void GetRelativeWeights(std::vector<double> *s, std::vector<double> *w) const" in ref
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_pose_graph_robust:" in mk and "all: build/test_pose_graph_robust\n" in mk
    abi = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("int ba_pgraph_set_robust(ba_pgraph *g", "int ba_pgraph_robust_check(int64_t n_rel",
                 "int ba_pgraph_factor_report(ba_pgraph *g", "(Triggs) correction"):
        assert name in abi, name


@pytest.mark.gpu
def test_cpp_robust_pose_graph_matches_the_direct_call_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_pose_graph_robust")
    assert os.path.exists(exe), "cpp/build/test_pose_graph_robust is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "POSE GRAPH ROBUST FACADE TEST PASSED" in r.stdout, r.stdout
