"""CPU: the FAST score network of csrc/orbx_fast_network.h equals the sixteen-arc definition of the segment test.

tests/fast_network_check.cpp is a stand-alone host program (its own main, not loaded into Python): it instantiates the header -
the same text the kernels compile - on plain integers, is built here with -fsanitize=address,undefined and run directly.  It
compares A = min over the 16 nine-arcs of the arc's maximum and B = max over the arcs of the arc's minimum, as the network gives
them, with two literal loops over the arcs, on

  * all 65 536 rings of values from {0,1}.  This is a PROOF, not a sample: network and definition are both built from min and max
    alone, i.e. they are lattice polynomials over a total order.  For any threshold t the map x -> [x >= t] commutes with min and
    max, so it commutes with both expressions.  If they differed on some ring p, say f(p) < g(p), then thresholding p at t = g(p)
    gives a 0/1 ring on which f is 0 and g is 1.  So agreement on every 0/1 ring is agreement everywhere;
  * 10^6 random rings of values 0..255 from a fixed seed: the values the kernels feed it, and a check of the check."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_network_equals_sixteen_arc_definition(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fast_network_check")
    # the sanitizer runtimes linked into the program (clang's default; g++ would otherwise take the shared ones, which insist on
    # being the first library of the process)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx) == "g++" else []
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror"] + static + [
           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "csrc"), os.path.join(ROOT, "tests", "fast_network_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "binary rings: 65536 ok" in r.stdout and "random rings: 1000000 ok" in r.stdout
