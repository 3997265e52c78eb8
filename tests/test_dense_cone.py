"""Host-only check of the cone sweep's lists (csrc/ba_dense_sched.cpp dense_cone_lists and
the back_cone decision of dense_launch_plan): the backward sweep of the reduced solve in
which the workgroup of a leaf tile solves its own chain of ancestors (k_chol_back_cone)
instead of waiting for other workgroups.  tests/cpp/dense_cone_check.cpp is compiled with
g++ against the planner source (no GPU, no HIP); its header lists what it asserts."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bundle_adjustment_solver_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                              "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_cone_lists_and_decision(tmp_path, flags):
    """Leaves, cones (closed, descending), row-tile slots, one writer per position, the
    decision against the caps, and the pinned figures of the 199-tile chain (100 leaves,
    longest cone 6, 572 steps on 196 non-tail tiles); once more as a stand-alone program
    under AddressSanitizer and UBSan."""
    exe = str(tmp_path / "dense_cone_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + flags +
                   [os.path.join(ROOT, "tests", "cpp", "dense_cone_check.cpp"),
                    os.path.join(CSRC, "ba_dense_sched.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "DENSE CONE CHECK OK" in r.stdout, r.stdout[-3000:]
