"""CPU (no GPU, no HIP call): orbx_level0_layout - where a caller of orbx_extract_batch_device_padded puts its frames - is level 0 of
what plan_size decides for the size, read through the developer build's orbx_debug_size_plan, and it refuses what plan_size refuses.

Sizes: the BASELINE.md sizes (640x480, 1241x376, 752x480, 1920x1080) and, next to each, the three widths that follow it, so that
w % 4 takes every value (the row misalignment (19 + w) % 4 the staging loops of the kernels meet); the shapes of the GPU test
(tests/test_level0_in_place_gpu.py: 252..255 x 190, 4 levels); the levels and scale factors a handle may have."""
import ctypes as C

import pytest

EDGE = 19
BASE = [(640, 480), (1241, 376), (752, 480), (1920, 1080)]
SIZES = sorted({(w + d, h) for w, h in BASE for d in range(4)})
assert {w % 4 for w, _ in SIZES} == {0, 1, 2, 3}


@pytest.fixture(scope="module")
def built(pkg):
    __import__("importlib").import_module("orb_slam2v2-1_amd.build").build()
    return pkg


def _level0(pkg, w, h, nlevels, scale, nfeatures=1000):
    d = pkg.debug_size_plan(nfeatures, scale, nlevels, w, h)
    assert d["status"] == pkg.ORBX_OK, d["message"]
    return d["geom"][0]


@pytest.mark.parametrize("nlevels,scale", [(8, 1.2), (4, 1.2), (1, 1.2), (3, 2.0), (8, 1.1)])
def test_layout_is_level_0_of_the_size_plan(built, nlevels, scale):
    pkg = built
    # (the 190-row shapes have room for four levels at 1.2: beyond, their coarsest level is smaller than a FAST cell - refused, see below)
    small = [(252, 190), (253, 190), (254, 190), (255, 190)] if (nlevels, scale) in ((4, 1.2), (1, 1.2)) else []
    for w, h in SIZES + small:
        g = _level0(pkg, w, h, nlevels, scale)
        lay = pkg.level0_layout(w, h, nlevels, scale)
        assert lay["pstride"] == int(g["pstride"]) and lay["prows"] == int(g["prows"]), (w, h, lay)
        assert int(g["w"]) == w and int(g["h"]) == h and int(g["poff"]) == 0
        assert lay["pixel0_offset"] == int(g["poff"]) + EDGE * int(g["pstride"]) + EDGE
        # what the kernels rely on: rows with one common misalignment, a frame of 19 px on every side inside the row
        assert lay["pstride"] % 64 == 0 and lay["pstride"] >= w + 2 * EDGE and lay["prows"] == h + 2 * EDGE
        # an image: the padded level, at least 16 bytes of slack behind its last dword, 256-byte granules like the pyramid block's images
        assert lay["image_bytes"] % 256 == 0 and lay["pstride"] * lay["prows"] + 16 <= lay["image_bytes"] < lay["pstride"] * lay["prows"] + 64 + 256
        # the feature budget does not move level 0 (it only sizes the quad-tree's LDS, which is the handle's to be refused for)
        g2 = _level0(pkg, w, h, nlevels, scale, nfeatures=300)
        assert (int(g2["pstride"]), int(g2["prows"]), int(g2["poff"])) == (int(g["pstride"]), int(g["prows"]), int(g["poff"]))
    # the developer build exports the same function
    assert pkg.level0_layout(1241, 376, nlevels, scale, developer=True) == pkg.level0_layout(1241, 376, nlevels, scale)


@pytest.mark.parametrize("w,h,nlevels,scale", [
    (60, 60, 1, 1.2),        # (w - 32) < 30: no FAST cell (ORBX_ERR_ARG)
    (252, 190, 8, 1.2),      # fine at level 0, the coarsest level has no FAST cell
    (5000, 400, 1, 1.2),     # coordinates are packed in 12 bits (ORBX_ERR_UNSUPPORTED)
    (400, 5000, 2, 1.2),
    (4000, 70, 1, 1.2),      # more quad-tree roots than the kernels take
])
def test_layout_refuses_what_plan_size_refuses(built, w, h, nlevels, scale):
    pkg = built
    d = pkg.debug_size_plan(1000, scale, nlevels, w, h)
    assert d["status"] in (pkg.ORBX_ERR_ARG, pkg.ORBX_ERR_UNSUPPORTED), d["status"]
    with pytest.raises(pkg.OrbxError) as e:
        pkg.level0_layout(w, h, nlevels, scale)
    assert e.value.status == d["status"]
    assert d["message"] and d["message"] in str(e.value)


def test_form_hook_is_declared_exported_by_the_developer_build_only(built):
    """include/orbx_dev_level0.h declares exactly the hooks of DEV_LEVEL0_EXPORTS; the developer library exports them, the product one
    does not (tests/test_abi_cpu.py holds the same for the hooks orbx_dev.h declares itself), and orbx_dev.h brings the header along."""
    import os
    import re
    import subprocess
    pkg = built
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "orbx_dev_level0.h")).read(), flags=re.S)
    decl = sorted(set(re.findall(r"\b(orb[xmv]_[a-z0-9_]+)\s*\(", txt)))
    assert decl == sorted(pkg.DEV_LEVEL0_EXPORTS) == ["orbx_debug_level0_in_place"]
    assert '#include "orbx_dev_level0.h"' in open(os.path.join(inc, "orbx_dev.h")).read()
    dev = subprocess.run(["nm", "-D", "--defined-only", pkg.DEV_LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    prod = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    for n in decl:
        assert re.search(r"\b%s\b" % n, dev) and hasattr(pkg.lib(True), n), n
        assert not re.search(r"\b%s\b" % n, prod), n
    # the product surface of the change is exported by both
    for n in ("orbx_level0_layout", "orbx_extract_batch_device_padded", "orbx_extract_batch_device_padded_prefetch"):
        assert n in pkg.EXPORTS and re.search(r"\b%s\b" % n, dev) and re.search(r"\b%s\b" % n, prod), n


def test_layout_argument_errors_and_accepted_sizes_agree(built):
    pkg = built
    L = pkg.lib()
    out = pkg.Level0Layout()
    for bad in ((640, 480, 0, 1.2), (640, 480, 17, 1.2), (640, 480, 8, 1.0)):
        assert L.orbx_level0_layout(*bad, C.byref(out)) == pkg.ORBX_ERR_ARG
    assert L.orbx_level0_layout(640, 480, 8, 1.2, None) == pkg.ORBX_ERR_ARG
    # every size the plan accepts for the usual handle gets a layout
    for w, h in SIZES:
        assert pkg.debug_size_plan(1000, 1.2, 8, w, h)["status"] == pkg.ORBX_OK
        assert L.orbx_level0_layout(w, h, 8, 1.2, C.byref(out)) == pkg.ORBX_OK
