"""CPU (no GPU; the static-count test needs the gfx950 cross compiler like the build): the records k_pyr_level's waves read instead of
deriving their set-up (csrc/orbx_size_plan.h: plan_pyr_records), through the developer build's orbx_debug_pyr_records.

A. every record against a restatement in numpy from the resize tables of the plan (xofsOff / xalphaOff / yofsOff / ybetaOff, geom): the
   column records field for field, the band records of both forms field for field, the "regular" flag by the rule the kernel evaluated
   per wave before the records existed (lane i of a band: its row's two source rows exist unclamped, lie within the SR rows fetched up
   front, and differ from the row above's; the ballot over the band's lanes);
B. the padded lane slots store nothing and read inside the source row;
C. the hook is a pure function of the size: 641x479, 258x255 and 641x479 again give what a first call gives (the same sequence on ONE
   handle, read back from its device buffers, is tests/test_pyr_level_records_gpu.py: a handle needs a GPU);
D. static counts of the two instances in the listing the build's flags give (helper copied from tests/test_address_counts_cpu.py).
   VALU instructions before the first source-row load, measured on the listing: parent 137 (<16,22>) and 132 (<8,12>), with the records
   18 and 18.  NumVgprs parent 52 / 32, with the records 51 / 31.  Whole kernel, static VALU: parent 540 / 345, now 445 / 265; an
   executed output row of the fast path is 10 VALU instructions (v_readlane of the row's betas, 4 v_mul_hi_u32_u24, 2 v_add3, shift,
   shift, v_and_or) against 13."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
EDGE = 19
HEAD = 8
SR_OF = {8: 12, 16: 22}
PARENT_SETUP_VALU = {16: 137, 8: 132}
PARENT_VGPRS = {16: 52, 8: 32}

CASES = [(1241, 376, 8, 1.2), (752, 480, 8, 1.2), (641, 479, 8, 1.2), (258, 255, 6, 1.2), (770, 431, 9, 1.1), (500, 400, 4, 1.25),
         (500, 400, 4, 1.3), (1023, 517, 5, 1.5)]
IDS = ["%dx%d_%d_%g" % c for c in CASES]


@pytest.fixture(scope="module")
def built(pkg):
    __import__("importlib").import_module("orb_slam2v2-1_amd.build").build()
    out = {}
    for c in CASES:
        w, h, nl, sf = c
        plan, rec = pkg.debug_size_plan(1000, sf, nl, w, h), pkg.debug_pyr_records(1000, sf, nl, w, h)
        assert plan["status"] == 0 and rec["status"] == 0, (c, plan["message"], rec["message"])
        out[c] = (plan, rec)
    return out


def _tables(plan, l):
    g, tab = plan["geom"][l], plan["tab"]
    w, h = int(g["w"]), int(g["h"])
    return (tab[int(g["xofsOff"]):int(g["xofsOff"]) + w].astype(np.int64), tab[int(g["xalphaOff"]):int(g["xalphaOff"]) + w].view(np.uint32),
            tab[int(g["yofsOff"]):int(g["yofsOff"]) + h].astype(np.int64), tab[int(g["ybetaOff"]):int(g["ybetaOff"]) + h].view(np.uint32))


def _expected_cols(plan, l):
    w = int(plan["geom"][l]["w"])
    xofs, xalpha, _, _ = _tables(plan, l)
    nxc = (w + 1 + 127) // 128
    x0 = 2 * np.arange(nxc * 64, dtype=np.int64) - 1
    xa, xb = np.clip(x0, 0, w - 1), np.minimum(x0 + 1, w - 1)
    ca, cb = EDGE + xofs[xa], EDGE + xofs[xb]
    A = ca & ~3
    sel = (ca - A) | ((cb - A) << 8) | ((x0 < w).astype(np.int64) << 16)
    return nxc, x0, np.stack([A, sel, xalpha[xa].astype(np.int64), xalpha[xb].astype(np.int64)], axis=1).astype(np.uint32)


def _expected_band(plan, l, RW, band):
    """(record words, regular) of one band by the kernel's former per-wave rule: lane i < RW holds the row table of output row y0 + i"""
    g, s = plan["geom"][l], plan["geom"][l - 1]
    h, sh, SR = int(g["h"]), int(s["h"]), SR_OF[RW]
    _, _, yofs, ybeta = _tables(plan, l)
    y0 = band * RW
    nrow = min(RW, h - y0)
    i = np.arange(RW)
    yl = np.minimum(y0 + i, h - 1)
    vsy, vbt = yofs[yl], ybeta[yl]
    rf = int(vsy[0])
    kk = vsy + 1 - rf
    prevsy = np.concatenate([vsy[:1], vsy[:-1]])
    okl = (i >= nrow) | ((rf >= 0) & (vsy + 1 <= sh - 1) & (kk < SR) & ((i == 0) | (vsy > prevsy)))
    regular = bool(okl.all())
    rec = np.zeros(HEAD + SR, np.uint32)
    rec[0], rec[3] = np.uint32(rf & 0xFFFFFFFF), nrow
    rec[5] = (EDGE + y0) * int(g["pstride"]) + EDGE - 1
    if regular:
        mask = 0
        for r in range(nrow):
            mask |= 1 << (int(kk[r]) & 31)
            b0, b1 = int(vbt[r]) & 0xFFFF, int(vbt[r]) >> 16
            assert 0 <= b0 <= 2048 and 0 <= b1 <= 2048   # 12 bits each
            rec[HEAD + int(kk[r])] = (b0 << 12) | b1
        rec[1], rec[2], rec[4] = mask, (mask | 1).bit_length() - 1, 1
        rec[6] = rf * int(s["pstride"])
    return rec, regular


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_records_equal_the_numpy_restatement(built, case):
    w, h, nl, sf = case
    plan, rec = built[case]
    ncols, nwords, irregular, edge_irregular = 0, 0, 0, 0
    for l in range(1, nl):
        g = plan["geom"][l]
        nxc, _, cols = _expected_cols(plan, l)
        assert rec["nxc"][l] == nxc and rec["colOff"][l] == ncols, l
        np.testing.assert_array_equal(rec["cols"][ncols:ncols + nxc * 64], cols, err_msg="level %d" % l)
        ncols += nxc * 64
        for f, RW in enumerate((8, 16)):
            if RW == 16 and sf > 1.25:
                assert rec["bandOff"][f][l] == -1 and rec["nbands"][f][l] == 0
                continue
            nb, words = (int(g["h"]) + RW - 1) // RW, HEAD + SR_OF[RW]
            assert rec["nbands"][f][l] == nb and rec["bandOff"][f][l] == nwords, (l, RW)
            for band in range(nb):
                exp, regular = _expected_band(plan, l, RW, band)
                got = rec["bands"][nwords + band * words:nwords + (band + 1) * words]
                np.testing.assert_array_equal(got, exp, err_msg="level %d form %d band %d" % (l, RW, band))
                irregular += not regular
                edge_irregular += (not regular) and band in (0, nb - 1)
            nwords += nb * words
    # lane i of a wave loads word i of its band record: the table ends with a wave's worth of zero words, so the last record's wave stays inside
    assert len(rec["cols"]) == ncols and len(rec["bands"]) == nwords + 64 and not rec["bands"][nwords:].any()
    assert (rec["bandOff"][:, 0] == -1).all() and (rec["bandOff"][:, nl:] == -1).all()
    print(case, "column records", ncols, "band words", nwords, "irregular bands", irregular, "of them first / last bands", edge_irregular)
    if sf > 1.25:
        assert (rec["bandOff"][1] == -1).all()   # no 16-row records: launch_pyramid never picks that form there
    if case == CASES[-1]:   # the row-by-row path stays covered: by the rule restated above, not by what the library flagged
        assert irregular >= 1
    # The first and the last band of every level are compared like every other band.  By the kernel's rule none of them is irregular at
    # any of these sizes (measured: 0 of them in all eight cases, 31 irregular bands at 1.5, all in between): a level is scaled DOWN, so
    # row 0 reads source rows 0 and 1 (fy = s / 2 - 1 / 2 >= 0) and the last row reads sh - 2 and sh - 1 (s > 1), never a clamped one.
    # What sends a band down the row-by-row path is its span of source rows (kk >= SR), which the 1.5 case has in the middle of a level.
    assert edge_irregular == 0 or sf > 1.25


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_padding_slots_store_nothing_and_read_inside_the_source_row(built, case):
    w, h, nl, sf = case
    plan, rec = built[case]
    for l in range(1, nl):
        lw, sps = int(plan["geom"][l]["w"]), int(plan["geom"][l - 1]["pstride"])
        nxc = int(rec["nxc"][l])
        cols = rec["cols"][int(rec["colOff"][l]):int(rec["colOff"][l]) + nxc * 64].astype(np.int64)
        assert len(cols) % 64 == 0 and len(cols) == nxc * 64 and 2 * len(cols) - 1 >= lw + 1   # whole waves that reach column w
        x0 = 2 * np.arange(len(cols)) - 1
        valid = (cols[:, 1] >> 16) & 1
        assert (valid == (x0 < lw)).all() and ((cols[:, 1] >> 17) == 0).all()
        pad = x0 >= lw
        assert pad.any() and (valid[pad] == 0).all()
        assert (cols[:, 0] % 4 == 0).all() and (cols[:, 0] + 8 <= sps).all(), l        # the 8-byte load of every slot, padded ones included
        oa, ob = cols[:, 1] & 0xFF, (cols[:, 1] >> 8) & 0xFF
        assert (oa + 1 < 8).all() and (ob + 1 < 8).all()                                # both byte pairs inside [A, A + 8)


def test_the_hook_is_a_pure_function_of_the_size(pkg, built):
    first = {}
    for (w, h) in ((641, 479), (258, 255), (641, 479)):
        r = pkg.debug_pyr_records(1000, 1.2, 6, w, h)
        assert r["status"] == 0
        if (w, h) in first:
            for k in ("cols", "bands", "nxc", "colOff", "nbands", "bandOff"):
                np.testing.assert_array_equal(r[k], first[(w, h)][k], err_msg=k)
        first[(w, h)] = r
    assert len(first[(641, 479)]["cols"]) != len(first[(258, 255)]["cols"])
    bad = pkg.debug_pyr_records(1000, 1.2, 8, 100, 100)   # refused like ensure_plan refuses it
    assert bad["status"] == pkg.ORBX_ERR_ARG and "cols" not in bad


# ---- static counts: the listing as tests/test_address_counts_cpu.py builds it (helper copied from there)
K_LEVEL = {16: "_Z11k_pyr_levelILi16ELi22EE", 8: "_Z11k_pyr_levelILi8ELi12EE"}


def _disassemble(tmp, src):
    out = os.path.join(tmp, src.replace(".hip", ".s"))
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-I" + os.path.join(tmp, "include"),
           "-I" + os.path.join(tmp, "orb_slam2v2-1_amd", "csrc"), "--cuda-device-only", "-S", "-o", out,
           os.path.join(tmp, "orb_slam2v2-1_amd", "csrc", src)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        return f.read().splitlines()


def _kernel(lines, prefix):
    """(instruction lines, resource comments) of the one kernel whose symbol starts with `prefix`"""
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


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("pyr_records"))
    for d in ("include", os.path.join("orb_slam2v2-1_amd", "csrc")):
        shutil.copytree(os.path.join(ROOT, d), os.path.join(tmp, d))
    return _disassemble(tmp, "orbx_pyramid.hip")


@pytest.mark.parametrize("RW", [16, 8])
def test_set_up_is_at_most_half_the_parents(listing, RW):
    body, res = _kernel(listing, K_LEVEL[RW])
    first = next(i for i, op in enumerate(body) if op.startswith("buffer_load_dwordx2"))   # the first source-row load
    setup = sum(1 for op in body[:first] if op.startswith("v_"))
    total = sum(1 for op in body if op.startswith("v_"))
    print("k_pyr_level<%d,%d>: VALU before the first source-row load %d (parent %d), static VALU %d, %s" % (RW, SR_OF[RW], setup, PARENT_SETUP_VALU[RW], total, res))
    assert 2 * setup <= PARENT_SETUP_VALU[RW]
    assert res["NumVgprs"] <= PARENT_VGPRS[RW] and res["ScratchSize"] == 0
    # the shuffles and the ballot's lane count are gone from the whole kernel, the division from the vector ALU
    for op in ("ds_bpermute_b32", "ds_swizzle_b32", "v_rcp_iflag_f32_e32", "v_mbcnt_lo_u32_b32"):
        assert op not in body, op
