"""The C++ facades' pose-graph optimisation (cpp/tests/test_pose_graph.cpp): SolvePoseGraph of
FullBundleAdjustmentSolver and FullBundleAdjustmentSolverRefactor in the caller's units against
ba_pgraph_create + ba_pgraph_solve called directly through include/ba_hip.h in scaled units, to
the bit; no camera, point or FinalizeParameters is needed; a finalized problem of the same
solver takes the new poses with ReloadParameterValues and Solve runs from them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "cpp")


def test_solve_pose_graph_is_declared_and_hooked_into_the_makefiles():
    hdr = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver.h")).read()
    assert "bool SolvePoseGraph(Options options, Summary *summary = nullptr);" in hdr
    ref = open(os.path.join(CPP, "include", "core", "full_bundle_adjustment_solver_refactor.h")).read()
    assert "bool SolvePoseGraph(Options options, Summary *summary = nullptr);" in ref
    mk = open(os.path.join(CPP, "Makefile")).read()
    assert "build/test_pose_graph:" in mk and "all: build/test_pose_graph\n" in mk
    lib_mk = open(os.path.join(ROOT, "bundle_adjustment_solver_amd", "csrc", "Makefile")).read()
    assert "ba_pgraph.o" in lib_mk and "ba_pgraph_host.h" in lib_mk
    abi = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    for name in ("int ba_pgraph_create(ba_pgraph **out, ba_handle *h", "void ba_pgraph_destroy(ba_pgraph *g)",
                 "int ba_pgraph_update_values(ba_pgraph *g", "int ba_pgraph_solve(ba_pgraph *g",
                 "int ba_pgraph_get_poses(ba_pgraph *g", "int ba_pgraph_cost(ba_pgraph *g",
                 "int ba_pgraph_get_system(ba_pgraph *g", "int ba_pgraph_info(ba_pgraph *g",
                 "int ba_pgraph_last_ms(ba_pgraph *g", "int ba_pgraph_check(int n_pose"):
        assert name in abi, name


@pytest.mark.gpu
def test_cpp_solve_pose_graph_matches_the_direct_call_on_gpu(built):
    exe = os.path.join(CPP, "build", "test_pose_graph")
    assert os.path.exists(exe), "cpp/build/test_pose_graph is not built (build() makes it)"
    r = subprocess.run([exe], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "POSE GRAPH FACADE TEST PASSED" in r.stdout, r.stdout
