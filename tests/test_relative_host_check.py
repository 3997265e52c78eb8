"""Host-only check of the relative-pose factors' host side (csrc/ba_rel_host.h): the rules
for the caller's arrays, the packing of the values and the one list builder that the planner,
the batch path and the pose graph share, against a brute-force statement of the lists in both
block-key conventions.  tools/relative_host_check.cpp is compiled with g++ under the address
and undefined-behaviour sanitizers as a stand-alone program (no GPU, no HIP, no Python in it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_relative_host_check_under_sanitizers(tmp_path):
    exe = str(tmp_path / "relative_host_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "relative_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("RELATIVE HOST CHECK PASSED"), r.stdout
