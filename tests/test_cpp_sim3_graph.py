"""The C++ facades' Sim(3) pose graph (cpp/tests/test_sim3_graph.cpp): AddRelativeSim3 and
SolveSim3Graph of FullBundleAdjustmentSolver and FullBundleAdjustmentSolverRefactor in the
caller's units against ba_sim3_create + ba_sim3_solve called directly through include/ba_hip.h in
scaled units, to the bit; rigid written-back poses, anchored points that keep their projections,
scales that recover the injected drift; SolvePoseGraph beside Sim(3) factors ignores them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_solve_sim3_graph_is_declared_and_hooked_into_the_makefiles():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    for text in (hdr, ref):
        assert "bool SolveSim3Graph(Options options, Summary *summary = nullptr, " \
               "const std::vector<int> *point_anchors = nullptr," in text
        assert "void AddRelativeSim3(const RelativeSim3 &factor, double sigma_pixel = 1.0)" in text
    assert "struct RelativeSim3 {" in hdr
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_sim3_graph:" in mk and "all: build/test_sim3_graph\n" in mk
    lib_mk = open(os.path.join(ROOT, "bundle_adjustment_solver_amd", "csrc", "Makefile")).read()
    assert "ba_sim3.o" in lib_mk and "ba_sim3_host.h" in lib_mk and "ba_sim3_fn.h" in lib_mk
    abi = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("int ba_sim3_create(ba_sim3 **out, ba_handle *h", "void ba_sim3_destroy(ba_sim3 *g)",
                 "int ba_sim3_update_values(ba_sim3 *g", "int ba_sim3_solve(ba_sim3 *g",
                 "int ba_sim3_get_poses(ba_sim3 *g", "int ba_sim3_cost(ba_sim3 *g",
                 "int ba_sim3_get_system(ba_sim3 *g", "int ba_sim3_factor_report(ba_sim3 *g",
                 "int ba_sim3_info(ba_sim3 *g", "int ba_sim3_last_ms(ba_sim3 *g", "int ba_sim3_check(int n_pose",
                 "void ba_sim3_exp(", "void ba_sim3_log(", "void ba_sim3_adjoint("):
        assert name in abi, name


@pytest.mark.gpu
def test_cpp_solve_sim3_graph_matches_the_direct_call_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_sim3_graph")
    assert os.path.exists(exe), "cpp/build/test_sim3_graph is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "SIM3 GRAPH FACADE TEST PASSED" in r.stdout, r.stdout
