"""GPU: the FAST score network (csrc/orbx_fast_network.h, 58 pinned packed operations per pixel pair) in every FAST kernel form,
bit for bit against the oracle, on an image made for it.

The image: 220x140, 2 levels, flat background, one synthetic ring per centre of a 10-px grid.  A centre's ring has a RUN of
consecutive ring pixels that are beyond the centre by more than iniThFAST, all brighter or all darker; the 128 centres cover both
polarities x every start position 0..15 x run lengths 8, 9, 10 and 16.  The values inside a run are pairwise distinct, so the
score depends on WHICH nine-arc wins; the ring pixels outside the run stay within 5 grey levels of the centre (below minThFAST).
FAST-9 must find the centres of length >= 9 and none of length 8: that is checked on the CPU, on the oracle's candidate list,
before any GPU call, so the comparison cannot pass on empty lists.  (Rings do not interact: 10-px grid, radius 3, and a ring
pixel's own ring reaches 6 px from the centre.)  The second image is uniform noise of the same size, where nearly every pixel
has a score.

Forms: B = 1 (k_fast_cells), the smallest batch the launch rule gives to k_fast_strips (asserted through orbx_debug_last_plan),
and the three corner-sparse forms by their option keys (row skip in k_fast_strips, k_fast_strips_sparse, k_fast_cells<.., true>)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, NF, NL, INI, MIN = 220, 140, 500, 2, 20, 7
BG = 100
MINB = 16   # EDGE_THRESHOLD - 3: candidate coordinates are relative to it
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
        (-2, 2), (-1, 3)]   # (dx, dy) of cv::FAST's 16-pixel circle, in its order
LENGTHS = (8, 9, 10, 16)


def ring_image():
    """-> (image, [(x, y, run length)] of the 128 centres)"""
    img = np.full((H, W), BG, np.uint8)
    rng = np.random.default_rng(58)
    centres = []
    n = 0
    for pol in (1, -1):
        for start in range(16):
            for L in LENGTHS:
                cx, cy = 25 + 10 * (n % 18), 25 + 10 * (n // 18)
                n += 1
                for pos, (dx, dy) in enumerate(RING):
                    if (pos - start) % 16 < L:   # inside the run: beyond the centre by 21 .. 66, distinct per ring position
                        v = BG + pol * (INI + 1 + 3 * ((pos * 7 + start * 3 + L) % 16))
                    else:
                        v = BG + int(rng.integers(-5, 6))
                    img[cy + dy, cx + dx] = v
                centres.append((cx, cy, L))
    assert n == 128 and cy + 3 < H - MINB - 3 and 25 + 10 * 17 + 3 < W - MINB - 3
    return img, centres


def build_cases(oracle):
    """The two images with the oracle's results: name -> (image, keypoints, descriptors, candidates per level, quad-tree keys per
    level).  The ring image's expectation is checked here, on the CPU."""
    rings, centres = ring_image()
    noise = np.random.default_rng(59).integers(0, 256, (H, W), dtype=np.uint8)
    out = {}
    for name, img in (("rings", rings), ("noise", noise)):
        orc = oracle.Extractor(NF, 1.2, NL, INI, MIN)
        k, d = orc.extract(img)
        out[name] = (img, k, d, [_cands(orc.level_candidates(l)) for l in range(NL)], [_cands(orc.level_keypoints(l)) for l in range(NL)])
    found = {(int(x) + MINB, int(y) + MINB): int(s) for x, y, s in out["rings"][3][0]}
    for cx, cy, L in centres:
        if L >= 9:
            assert found.get((cx, cy), 0) >= INI, ("no candidate at a centre with a run of %d" % L, cx, cy)
        else:
            assert (cx, cy) not in found, ("candidate at a centre with a run of 8", cx, cy)
    assert len(out["noise"][3][0]) > 100 and len(out["noise"][1]) > 100
    return out


@pytest.fixture(scope="module")
def cases(oracle):
    return build_cases(oracle)   # computed once, shared, never written to


def _cands(a):
    return np.stack([a["x"], a["y"], a["score"]], 1).astype(np.int32) if len(a) else np.zeros((0, 3), np.int32)


def _check_levels(ex, case, b=0, what=""):
    for l in range(NL):
        np.testing.assert_array_equal(ex.debug_level_points(l, 0, b), case[3][l], err_msg="FAST candidates level %d %s" % (l, what))
        np.testing.assert_array_equal(ex.debug_level_points(l, 1, b), case[4][l], err_msg="quad-tree level %d %s" % (l, what))


def _check_final(gk, gd, case, what=""):
    ok, od = case[1], case[2]
    assert len(gk) == len(ok), what
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        np.testing.assert_array_equal(gk[f], ok[f], err_msg=f + " " + what)
    np.testing.assert_allclose(gk["angle"], ok["angle"], atol=1e-4, rtol=0)
    np.testing.assert_array_equal(gd, od, err_msg=what)


@pytest.mark.parametrize("name", ["rings", "noise"])
def test_cell_kernel_single_image(pkg, hooks, cases, name):
    ex = pkg.ORBextractor(NF, 1.2, NL, INI, MIN)
    gk, gd = ex(cases[name][0])
    p = ex.debug_last_plan()
    assert not p["strips"] and p["fastCells"], p
    _check_levels(ex, cases[name])
    _check_final(gk, gd, cases[name])
    ex.close()


def test_strip_kernel_smallest_batch(pkg, hooks, cases):
    """The launch rule hands the FAST stage to k_fast_strips once the strips of a batch fill the GPU: the smallest such batch of
    this image size, rings in the even slots and noise in the odd ones, and the batch one image short of it (cells)."""
    ex = pkg.ORBextractor(NF, 1.2, NL, INI, MIN)
    ex(cases["rings"][0])   # plans the size
    B = next(b for b in range(2, 4097) if "k_fast_strips" in ex.fast_kernels(b))
    assert "k_fast_strips" not in ex.fast_kernels(B - 1)
    names = ["rings", "noise"]
    imgs = np.stack([cases[names[b % 2]][0] for b in range(B)])
    got = ex.extract_batch(imgs)
    p = ex.debug_last_plan()
    assert p["strips"] and p["stripLevels"] == (1 << NL) - 1 and not p["fastCells"] and not p["compact"], (B, p)
    for b in (0, 1, B - 2, B - 1):
        _check_levels(ex, cases[names[b % 2]], b, "slot %d of %d" % (b, B))
    for b in range(B):
        _check_final(got[b][0], got[b][1], cases[names[b % 2]], "slot %d of %d" % (b, B))
    got = ex.extract_batch(imgs[:B - 1])
    p = ex.debug_last_plan()
    assert not p["strips"] and p["fastCells"], (B - 1, p)
    for b in (0, 1, B - 2):
        _check_final(got[b][0], got[b][1], cases[names[b % 2]], "slot %d of %d" % (b, B - 1))
    ex.close()


@pytest.mark.parametrize("name", ["rings", "noise"])
@pytest.mark.parametrize("form", [0, 1, 2], ids=["row_skip", "strip_compaction", "cell_compaction"])
def test_corner_sparse_forms(pkg, hooks, cases, name, form):
    """ORBX_OPT_FAST_FORM 3 (strips for one image), ORBX_OPT_ROW_PRETEST 2 (every level takes the sparse path) and the three
    ORBX_OPT_SPARSE_FORMs; the second call on the handle is the one that sees the first call's verdicts."""
    ex = pkg.ORBextractor(NF, 1.2, NL, INI, MIN)
    ex.set_option(6, 3)
    ex.set_option(16, 2)
    ex.set_option(20, form)
    for rep in range(2):
        gk, gd = ex(cases[name][0])
        p = ex.debug_last_plan()
        assert p["strips"] and p["rowFlags"] and p["sparseForm"] == form, p
        _check_levels(ex, cases[name], 0, "call %d" % rep)
        _check_final(gk, gd, cases[name], "call %d" % rep)
    ex.close()
