"""Host-only check of GraphSession<Abi> (cpp/include/core/graph_session.h), the owner of a pose
graph and its handle behind the graph methods of the C++ facade: with a fake traits type that counts
creates and destroys and fails on demand, the graph is destroyed exactly once if it was created, an
own handle exactly once and a borrowed handle never, and the thrown text is "<entry>: <error>" as
the error stood before any destroy.  tools/graph_session_host_check.cpp is compiled with g++ as a
stand-alone program (no GPU, no HIP, no library, no Python in it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graph_session_host_check(tmp_path):
    exe = str(tmp_path / "graph_session_host_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-I" + os.path.join(ROOT, "cpp", "include"),
                    os.path.join(ROOT, "tools", "graph_session_host_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("GRAPH SESSION HOST CHECK PASSED"), r.stdout
