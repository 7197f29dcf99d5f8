"""GPU: k_pyr_level reading its per-wave set-up from the records of the planned size (csrc/orbx_size_plan.h: plan_pyr_records) - every
padded level byte for byte against the CPU oracle, key points and descriptors equal, with ORBX_OPT_PYRAMID_FORM = 2 (single images
take k_pyr_level, not the chains) and ORBX_OPT_PYR_ROWS = 1 / 2 (k_pyr_level<8,12> / <16,22>).

The shapes are the smallest at which the new indexing can go wrong: level-1 widths 127 / 128 / 129 (the last 128-column chunk with one
valid lane slot, with none to spare, and a chunk that only holds the frame column x0 = w) crossed with level-1 heights 95 / 96 / 97
(bands of 15, 16 and 16 + 1 rows); the other scale factors (1.1: dense row masks, 1.25: the largest with the 16-row form, 1.3: the
8-row form whatever ORBX_OPT_PYR_ROWS says); a batch above ORBX_HIST_IMAGES (image stride), and the same batch around a call of
another size on one handle (the records are planned and uploaded again), with the handle's device copy of the records read back.
plan_size accepts every size used here as it stands."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NF = 500
OPT_PYRAMID_FORM, OPT_PYR_ROWS = 5, 22


@pytest.fixture(params=[1, 2], ids=["8_rows_per_wave", "16_rows_per_wave"])
def rows(request, pkg):
    pkg.set_default_option(OPT_PYRAMID_FORM, 2)
    pkg.set_default_option(OPT_PYR_ROWS, request.param)
    try:
        yield request.param
    finally:
        pkg.set_default_option(OPT_PYR_ROWS, 0)
        pkg.set_default_option(OPT_PYRAMID_FORM, 0)


def _single(pkg, oracle, img, nl, sf):
    h, w = img.shape
    ex = pkg.ORBextractor(NF, sf, nl, 20, 7)
    try:
        k, d = ex(img)
        o = oracle.Extractor(NF, sf, nl, 20, 7)
        ok, od = o.extract(img)
        for lvl in range(nl):
            np.testing.assert_array_equal(ex.pyramid_level(lvl, padded=True), o.pyramid_level(lvl, padded=True), err_msg=str((w, h, nl, sf, lvl)))
        assert k.tobytes() == ok.tobytes() and d.tobytes() == od.tobytes(), (w, h, nl, sf)
    finally:
        ex.close()


@pytest.mark.parametrize("h", [114, 115, 116])
@pytest.mark.parametrize("w", [152, 154, 155])
def test_level_1_on_both_sides_of_a_chunk_and_of_a_band(pkg, oracle, synth, rows, w, h):
    p = pkg.debug_size_plan(NF, 1.2, 2, w, h)
    assert p["status"] == 0, p["message"]
    assert (int(p["geom"][1]["w"]), int(p["geom"][1]["h"])) == ({152: 127, 154: 128, 155: 129}[w], {114: 95, 115: 96, 116: 97}[h])
    _single(pkg, oracle, synth.frame(w, h, 7000 + w * 3 + h), 2, 1.2)


@pytest.mark.parametrize("w,h,nl,sf", [(258, 255, 6, 1.2), (770, 431, 9, 1.1), (500, 400, 4, 1.25), (500, 400, 4, 1.3)])
def test_other_scale_factors(pkg, oracle, synth, rows, w, h, nl, sf):
    _single(pkg, oracle, synth.frame(w, h, 7100 + w + nl), nl, sf)


@pytest.fixture(scope="module")
def five(oracle, synth):
    """five distinct 258x255 images and the oracle's levels, key points and descriptors of each (computed once, read only)"""
    imgs = synth.batch(258, 255, 5, k0=7200)
    assert len({im.tobytes() for im in imgs}) == 5
    ref = []
    for im in imgs:
        o = oracle.Extractor(NF, 1.2, 6, 20, 7)
        k, d = o.extract(im)
        ref.append((k, d, [o.pyramid_level(l, padded=True).copy() for l in range(6)]))
    return imgs, ref


def _check_batch(ex, res, ref):
    for b, (k, d, levels) in enumerate(ref):
        for l, lv in enumerate(levels):
            np.testing.assert_array_equal(ex.pyramid_level(l, b=b, padded=True), lv, err_msg="image %d level %d" % (b, l))
        assert res[b][0].tobytes() == k.tobytes() and res[b][1].tobytes() == d.tobytes(), b


def test_batch_above_the_small_batch_limit(pkg, rows, five):
    imgs, ref = five
    ex = pkg.ORBextractor(NF, 1.2, 6, 20, 7)
    try:
        _check_batch(ex, ex.extract_batch(imgs), ref)
    finally:
        ex.close()


def _same_records(a, b):
    for k in ("cols", "bands", "nxc", "colOff", "nbands", "bandOff"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_one_handle_plans_and_uploads_the_records_again(pkg, oracle, synth, rows, five):
    """batch of 258x255, one 641x479 image, the batch again on ONE handle: results as before, and after every call the handle's device
    buffers hold exactly the records a first plan of that size gives"""
    imgs, ref = five
    big = synth.frame(641, 479, 7300)
    o = oracle.Extractor(NF, 1.2, 6, 20, 7)
    ok, od = o.extract(big)
    fresh = {s: pkg.debug_pyr_records(NF, 1.2, 6, s[0], s[1]) for s in ((258, 255), (641, 479))}
    assert fresh[(258, 255)]["status"] == 0 and fresh[(641, 479)]["status"] == 0
    ex = pkg.ORBextractor(NF, 1.2, 6, 20, 7, developer=True)
    try:
        _check_batch(ex, ex.extract_batch(imgs), ref)
        _same_records(pkg.debug_pyr_records(extractor=ex), fresh[(258, 255)])
        k, d = ex(big)
        for lvl in range(6):
            np.testing.assert_array_equal(ex.pyramid_level(lvl, padded=True), o.pyramid_level(lvl, padded=True), err_msg="641x479 level %d" % lvl)
        assert k.tobytes() == ok.tobytes() and d.tobytes() == od.tobytes()
        _same_records(pkg.debug_pyr_records(extractor=ex), fresh[(641, 479)])
        _check_batch(ex, ex.extract_batch(imgs), ref)
        _same_records(pkg.debug_pyr_records(extractor=ex), fresh[(258, 255)])
    finally:
        ex.close()
