"""CPU (no GPU; needs the gfx950 cross compiler like the build): the static instruction mix of k_describe's hot path.

tools/phase_count.py compiles orbx_describe.hip with -DORBX_PHASE_MARKERS and counts the instructions of k_describe<half_up, no split>
per phase from the disassembly.  The hot path is straight-line, so the static VALU count is the executed one.  Before the per-level
grid, the five-row staging rounds, the per-alignment horizontal pass and the wide record stores it was 533 VALU instructions per
keypoint wave (profiles/r04_describe_phase_counts.txt, profiles/describe_phase_counts.txt); the four changes were set targets of
29 + 22 + 13 + 18 = 82 fewer, and this test holds the kernel to at least 70 fewer (12 of margin for what the register allocator
gives back).  No item was left out, so the bar is the full one."""
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT_VALU = 533
BAR = 70


def test_describe_hot_path_valu_count(tmp_path):
    # a copy of the sources: the tool writes its disassembly under <root>/tools/_build
    for d in ("include", os.path.join("orb_slam2v2-1_amd", "csrc")):
        shutil.copytree(os.path.join(ROOT, d), str(tmp_path / d))
    os.makedirs(str(tmp_path / "tools"))
    shutil.copy(os.path.join(ROOT, "tools", "phase_count.py"), str(tmp_path / "tools" / "phase_count.py"))
    out = subprocess.run([sys.executable, str(tmp_path / "tools" / "phase_count.py"), "orbx_describe.hip", "_Z10k_describeILi0ELb0E"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    rows = {}
    for line in out.stdout.splitlines():
        m = re.match(r"(\S+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s*$", line)
        if m:
            rows[m.group(1)] = [int(v) for v in m.groups()[1:]]
    for phase in ("locate", "stage", "ic_angle", "horizontal", "vertical", "brief", "store", "total"):
        assert phase in rows, (phase, sorted(rows))
    assert rows["total"][0] == sum(v[0] for k, v in rows.items() if k != "total")
    assert rows["total"][0] <= PARENT_VALU - BAR, rows
