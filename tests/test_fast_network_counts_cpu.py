"""CPU (no GPU; needs the gfx950 cross compiler like the build): the FAST score network reaches the assembly with 58 packed
3-input minima / maxima per pixel-pair row, not 72.

Same method as test_address_counts_cpu.py: cross-compile a copy of the sources with the build's flags, with and without the phase
markers, and count opcodes in the disassembly.  Before the network of csrc/orbx_fast_network.h the same measurement gave for
k_fast_strips 1086 static VALU of which 672 v_pk_minimum3_f16 + v_pk_maximum3_f16 (8 unrolled rows x (72 + 4) for the score,
the rest the cold row pre-test, suppression and clamp) and 64 VGPRs, and for k_fast_cells<0,false> 154 packed minima / maxima.
With every operation of the network pinned to one instruction: 974 VALU, 560 packed (8 x 58 + 56 + 40), 52 VGPRs;
k_fast_cells<0,false> 126 (two score sites, 14 fewer each).  Written through the builtins the compiler re-associates the nested
maxima and recomputes the shared 3-windows: 1038 VALU, 624 packed.  The bars: 974 + the 10 that test_address_counts_cpu.py also
allows the register allocator; the 560 with no allowance (one recomputed 3-window per row shows as 8 more); at least 12 fewer in
the cell kernel."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

K_STRIPS = "_Z13k_fast_strips"
K_CELLS_RT = "_Z12k_fast_cellsILi0ELb0EE"
PARENT_CELLS_PK = 154


def _disassemble(tmp, markers):
    out = os.path.join(tmp, "orbx_fast_m.s" if markers else "orbx_fast.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-I" + os.path.join(tmp, "include"),
           "-I" + os.path.join(tmp, "orb_slam2v2-1_amd", "csrc"), "--cuda-device-only", "-S", "-o", out,
           os.path.join(tmp, "orb_slam2v2-1_amd", "csrc", "orbx_fast.hip")]
    if markers:
        cmd.append("-DORBX_PHASE_MARKERS")
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        return f.read().splitlines()


def _kernel(lines, prefix):
    """(opcodes, resource comments) of the one kernel whose symbol starts with `prefix`"""
    starts = [i for i, l in enumerate(lines) if l.startswith(prefix) and re.match(r"\S+:(\s|$)", l)]
    assert len(starts) == 1, (prefix, starts)
    end = next(i for i in range(starts[0], len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = []
    for l in lines[starts[0] + 1:end]:
        t = l.strip()
        if t and not t.startswith((";", ".", "//")) and not t.endswith(":"):
            body.append(t.split()[0])
    res = {}
    for l in lines[end:end + 80]:
        m = re.match(r";\s*(NumVgprs|ScratchSize):\s*(\d+)", l.strip())
        if m and m.group(1) not in res:
            res[m.group(1)] = int(m.group(2))
    assert set(res) == {"NumVgprs", "ScratchSize"}, res
    return body, res


def _valu(body):
    return sum(1 for op in body if op.startswith("v_"))


def _pk3(body):
    return sum(1 for op in body if re.sub(r"_e(32|64)$", "", op) in ("v_pk_minimum3_f16", "v_pk_maximum3_f16"))


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("fast_network_counts"))
    for d in ("include", os.path.join("orb_slam2v2-1_amd", "csrc")):
        shutil.copytree(os.path.join(ROOT, d), os.path.join(tmp, d))
    return {"markers": _disassemble(tmp, True), "plain": _disassemble(tmp, False)}


@pytest.mark.parametrize("build", ["markers", "plain"])
def test_fast_strips_network_counts(listings, build):
    body, res = _kernel(listings[build], K_STRIPS)
    valu, pk = _valu(body), _pk3(body)
    print("k_fast_strips (%s build): VALU %d, packed min3/max3 %d, %s" % (build, valu, pk, res))
    assert valu <= 984
    assert pk <= 560
    assert res["ScratchSize"] == 0 and res["NumVgprs"] <= 64


def test_fast_cells_network_counts(listings):
    body, res = _kernel(listings["plain"], K_CELLS_RT)
    pk = _pk3(body)
    print("k_fast_cells<0,false>: VALU %d, packed min3/max3 %d (was %d), %s" % (_valu(body), pk, PARENT_CELLS_PK, res))
    assert pk <= PARENT_CELLS_PK - 12
