"""Host-only check of the planner's part of the relative-pose factors on the handle path
(csrc/ba_plan.cpp: PlanInput::rel_j / rel_k): every factor pair of two optimisable poses is a
block of S exactly once, pairs in both orientations and duplicates share one block, a pair to
a fixed pose adds none, tile_pattern couples their tiles, the two lists are in input order,
and factors that add no block leave every other array of the plan as it was.
tests/cpp/rel_plan_check.cpp is compiled with g++ against the planner sources (no GPU, no HIP)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bundle_adjustment_solver_amd", "csrc")


@pytest.fixture(scope="module")
def rel_plan_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("relplan") / "rel_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "rel_plan_check.cpp"),
                    os.path.join(CSRC, "ba_plan.cpp"),
                    os.path.join(CSRC, "ba_dense_sched.cpp"), "-o", exe, "-pthread"], check=True)
    return exe


@pytest.mark.parametrize("args,env", [
    (["60", "3000", "5"], {}),                        # covisibility groups
    (["60", "3000", "5"], {"BA_NO_GROUPS": "1"}),     # super-runs only
    (["33", "700", "9"], {}),                         # wide windows, a pose count that is no multiple of a tile
    (["150", "9000", "5"], {}),
])
def test_relative_plan(rel_plan_check, args, env):
    r = subprocess.run([rel_plan_check] + args, env=dict(os.environ, **env),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout
