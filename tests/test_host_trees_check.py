"""The host tree builder (csrc/host_trees.cpp) stays a host-only unit: tools/host_trees_check.cpp, built here with the
host compiler alone (no HIP compiler, no HIP header on the include path, no sanitizer) and linked with nothing but the
builder and the host scene library's source, runs clean. The program checks the trees of generated scenes and of one
degenerate input (coincident centroids, which drive the depth cap): the partitions, containment, depth below the
traversal stack, and the raster tree's leaf ranges. Its header carries the sanitizer build line for the same sources."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "path-tracing-svgf_amd", "csrc")


def test_host_trees_check_builds_with_the_host_compiler_and_passes(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "host_trees_check")
    cmd = [cxx, "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I" + CSRC,
           os.path.join(REPO, "tools", "host_trees_check.cpp"), os.path.join(CSRC, "host_trees.cpp"),
           os.path.join(CSRC, "scene_prep.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "host_trees_check: ok" in r.stdout
