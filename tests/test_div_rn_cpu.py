"""CPU: orbx_div_rn, the FMA-free correctly rounded division of k_rect_map (orb_slam2v2-1_amd/csrc/orbx_div_rn.h), compiled for the
host and compared with x86 division bit for bit (tests/cpp/div_rn_check.cc): special operands, subnormal and overflowing quotients,
exact quotients and random operands."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_div_rn_equals_x86_division(tmp_path):
    exe = str(tmp_path / "div_rn_check")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "div_rn_check.cc")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    bad, n = (int(v) for v in out.stdout.split()[-2:])
    assert bad == 0 and n > 4000000
