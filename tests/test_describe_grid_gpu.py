"""GPU: k_describe's per-level grid (a describing block belongs to ONE level: DescGroup::blk0), the staging in rounds of five whole
rows, the four copies of the horizontal pass (one per patch alignment) and the wide record stores.

Every test compares keypoints, descriptors and counts with the oracle bit for bit (angles within 1e-4, as elsewhere) on images of at
most 640x480.  The conditions a case is about (a level whose count is no multiple of the waves of a block, an empty level in front
of a non-empty one, a capacity that ends inside a level, every patch alignment at every level, a keypoint on the edge path) are
computed from the oracle's per-level lists and ASSERTED, so that a changed image generator cannot silently void a case.
Reference: src/ORBextractor.cc:1076-1104 (level-major concatenation), :77-147."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DESC_WAVES = 4      # keypoints (waves) per describing block (csrc/orbx_extract_dev.h)
MINB = 16           # the level lists hold coordinates relative to the FAST border (EDGE_THRESHOLD - 3)
PR = 21             # radius of the patch k_describe stages: closer than that to a level's edge = the reflecting staging path


def _check(gk, gd, ok, od):
    assert len(gk) == len(ok), (len(gk), len(ok))
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        np.testing.assert_array_equal(gk[f], ok[f], err_msg=f)
    np.testing.assert_allclose(gk["angle"], ok["angle"], atol=1e-4, rtol=0)
    np.testing.assert_array_equal(gd, od)


def _blobs(seed, w=640, h=480, sigma=10.0, amp=60.0, n=40):
    """A flat image with one patch of smooth blobs: too gentle for FAST's radius-3 circle at the finest levels, corners further up."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 128.0)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n):
        cx, cy = rng.uniform(200, 440), rng.uniform(140, 340)
        s = sigma * rng.uniform(0.8, 1.6)
        img += amp * rng.choice([-1, 1]) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return np.clip(img + 0.5, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _small_frames():
    """Five 320x240 frames and what the oracle (default flavour, 400 features, 8 levels) makes of them: shared, never modified."""
    import importlib
    import oracle
    synth = importlib.import_module("orb_slam2v2-1_amd.synth")
    imgs = np.stack([synth.frame(320, 240, k=1 + i) for i in range(5)])
    orc = oracle.Extractor(400, 1.2, 8, 20, 7)
    exp, lists = [], []
    for im in imgs:
        exp.append(orc.extract(im))
        lists.append([(orc.level_keypoints(l).copy(), orc.pyramid_level(l).shape) for l in range(8)])
    return imgs, exp, lists


def _device_records(pkg, ex, imgs, cap):
    import torch
    B, h, w = imgs.shape
    d = torch.from_numpy(imgs).cuda()
    kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d.data_ptr(), B, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), cap, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    k = kps.cpu().numpy().view(np.uint8).reshape(B, cap, 28)
    return [np.frombuffer(k[b].tobytes(), pkg.KP_DTYPE) for b in range(B)], desc.cpu().numpy(), cnt.cpu().numpy()


def test_level_boundaries(pkg, oracle):
    """8 levels, 300 features, a flat image with one patch of smooth blobs: a level whose count is no multiple of the block's waves (its
    last block is partly empty) and an empty level in front of a non-empty one (blocks that return at once, the prefix goes on)."""
    img = _blobs(1)
    orc = oracle.Extractor(300, 1.2, 8, 20, 7)
    ok, od = orc.extract(img)
    counts = [len(orc.level_keypoints(l)) for l in range(8)]
    assert any(c % DESC_WAVES for c in counts), counts
    assert any(counts[l] == 0 and any(counts[l + 1:]) for l in range(7)), counts
    ex = pkg.ORBextractor(300, 1.2, 8, 20, 7)
    for _ in range(2):
        _check(*ex(img), ok, od)
    assert list(ex.level_counts()[1]) == counts


@pytest.mark.parametrize("nlevels,sf", [(1, 1.2), (16, 1.1)])
def test_level_count_extremes(pkg, oracle, synth, nlevels, sf):
    """One level (no entry of the block table is ever passed) and ORBX_MAX_LEVELS = 16 levels (every entry is one level's)."""
    img = synth.frame(640, 480, k=3)
    orc = oracle.Extractor(500, sf, nlevels, 20, 7)
    ok, od = orc.extract(img)
    counts = [len(orc.level_keypoints(l)) for l in range(nlevels)]
    assert all(counts), counts
    ex = pkg.ORBextractor(500, sf, nlevels, 20, 7)
    _check(*ex(img), ok, od)
    assert list(ex.level_counts()[1]) == counts


def test_cap_inside_a_level(pkg):
    """A caller's capacity below the total that ends strictly inside a level: the kept prefix and counts[b] are the oracle's first
    `cap` records, nothing is written behind them."""
    imgs, exp, lists = _small_frames()
    c0 = [len(lk) for lk, _ in lists[0]]
    cap = c0[0] + c0[1] + c0[2] // 2 + 1
    for b in range(2):
        pre = np.cumsum([len(lk) for lk, _ in lists[b]])
        assert cap < pre[-1] and cap not in pre and pre[1] < cap < pre[2], (b, cap, pre)
    ex = pkg.ORBextractor(400, 1.2, 8, 20, 7)
    kps, desc, cnt = _device_records(pkg, ex, imgs[:2], cap)
    for b in range(2):
        assert cnt[b] == cap
        _check(kps[b], desc[b], exp[b][0][:cap], exp[b][1][:cap])
    # a capacity above the total keeps everything and leaves the slots behind the list untouched
    full = ex.max_keypoints()
    kps, desc, cnt = _device_records(pkg, ex, imgs[:2], full)
    for b in range(2):
        n = len(exp[b][0])
        assert cnt[b] == n
        _check(kps[b][:n], desc[b][:n], *exp[b])
        assert not desc[b][n:].any() and not kps[b][n:].view(np.uint8).any()


def test_alignment_and_edges(pkg):
    """Every non-empty level keeps keypoints of all four patch alignments (byte of the patch origin inside its dword: the four copies
    of the horizontal pass), and a level >= 1 keeps a keypoint closer than 21 px to its edge (staged through reflected coordinates)."""
    imgs, exp, lists = _small_frames()
    nedge = 0
    for l, (lk, (lh, lw)) in enumerate(lists[0]):
        cx, cy = lk["x"] + MINB, lk["y"] + MINB
        edge = (l >= 1) & ((cx < PR) | (cy < PR) | (cx + PR >= lw) | (cy + PR >= lh))
        nedge += int(edge.sum())
        if len(lk):     # pstride is a multiple of 64: the alignment is that of column cx + 19 - 21 of the padded level
            assert set(((cx[~edge] - 2) & 3).tolist()) == {0, 1, 2, 3}, l
    assert nedge >= 1
    ex = pkg.ORBextractor(400, 1.2, 8, 20, 7)
    _check(*ex(imgs[0]), *exp[0])


@pytest.mark.parametrize("B", [1, 2, 5])
def test_batches(pkg, B):
    """Batch sizes with every remainder of the block -> (image, block) map over the eight L2s that a small grid can have."""
    imgs, exp, _ = _small_frames()
    ex = pkg.ORBextractor(400, 1.2, 8, 20, 7)
    got = ex.extract_batch(imgs[:B])
    for b in range(B):
        _check(*got[b], *exp[b])


def test_forms_split_call(pkg, hooks):
    """The two launches of a split call (levels [3, 8) into scratch arrays, then levels [0, 3) and the copy blocks), at the full capacity
    and at one that ends inside the first group."""
    imgs, exp, _ = _small_frames()
    batch = np.concatenate([imgs, imgs[:3]])      # a split call needs eight images
    ex = pkg.ORBextractor(400, 1.2, 8, 20, 7)
    usual = ex(imgs[0])
    _check(*usual, *exp[0])
    pkg.set_default_option(15, 3)
    try:
        for cap in (ex.max_keypoints(), 150):
            kps, desc, cnt = _device_records(pkg, ex, batch, cap)
            p = ex.debug_last_plan()
            assert p["aSplit"] == 3 and p["octForm"] == pkg.OCT_SPLIT, p
            for b in range(8):
                ok, od = exp[b % 5]
                n = min(len(ok), cap)
                assert cnt[b] == n
                _check(kps[b][:n], desc[b][:n], ok[:n], od[:n])
            if cap >= len(usual[0]):
                assert kps[0][:cnt[0]].tobytes() == usual[0].tobytes() and desc[0][:cnt[0]].tobytes() == usual[1].tobytes()
    finally:
        pkg.set_default_option(15, 0)


def test_forms_latency_view(pkg):
    """orbx_stereo_frame_view: k_describe repeats its stores in the record's pinned twin.  Both copies equal the usual launch's output."""
    imgs, exp, _ = _small_frames()
    ex = pkg.ORBextractor(400, 1.2, 8, 20, 7)
    usual = [ex(imgs[0]), ex(imgs[1])]
    f = ex.stereo_frame_view(imgs[0], imgs[1], 386.1448, float(np.float32(386.1448) / np.float32(718.856)))
    hip = C.CDLL("libamdhip64.so")
    v = f["view"]
    for side, (uk, ud), ok_od in (("l", usual[0], exp[0]), ("r", usual[1], exp[1])):
        pk, pd = f["k" + side], f["d" + side]
        _check(pk, pd, *ok_od)
        assert pk.tobytes() == uk.tobytes() and pd.tobytes() == ud.tobytes(), side
        n = len(pk)
        hk, hd = np.zeros(n, pkg.KP_DTYPE), np.zeros((n, 32), np.uint8)      # the same record in HBM
        assert hip.hipMemcpy(C.c_void_p(hk.ctypes.data), C.c_void_p(getattr(v, "d_k" + side)), C.c_size_t(n * 28), C.c_int(2)) == 0
        assert hip.hipMemcpy(C.c_void_p(hd.ctypes.data), C.c_void_p(getattr(v, "d_d" + side)), C.c_size_t(n * 32), C.c_int(2)) == 0
        assert hk.tobytes() == pk.tobytes() and hd.tobytes() == pd.tobytes(), side


@pytest.mark.parametrize("gauss", ["half_up", "sse2", "taps:55,49,34,18", "taps:56,48,34,18"])
def test_forms_gauss_flavours(pkg, oracle, gauss):
    """The three instances of the kernel (literal taps with either column rounding, the handle's taps), each against the oracle of its
    own flavour; keypoints do not depend on the flavour, and the handle's taps 55 49 34 18 ARE the half-up flavour, byte for byte."""
    imgs, exp, _ = _small_frames()
    img = imgs[0]
    ok, od = oracle.Extractor(400, 1.2, 8, 20, 7, gauss=gauss).extract(img)
    gk, gd = pkg.ORBextractor(400, 1.2, 8, 20, 7, gauss=gauss)(img)
    _check(gk, gd, ok, od)
    hk, hd = pkg.ORBextractor(400, 1.2, 8, 20, 7, gauss="half_up")(img)
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        np.testing.assert_array_equal(gk[f], hk[f], err_msg=f)
    if gauss in ("half_up", "taps:55,49,34,18"):
        assert gk.tobytes() == hk.tobytes() and gd.tobytes() == hd.tobytes()


def test_forms_level_wide_blur(pkg, hooks):
    """Developer knob 13 = 2: every level blurred as a whole, k_describe only gathers.  Equal to the usual launch's output."""
    imgs, exp, _ = _small_frames()
    ex = pkg.ORBextractor(400, 1.2, 8, 20, 7)
    usual = ex(imgs[0])
    ex.set_option(13, 2)
    gk, gd = ex(imgs[0])
    assert ex.blurred_mask() == 0xFF
    _check(gk, gd, *exp[0])
    assert gk.tobytes() == usual[0].tobytes() and gd.tobytes() == usual[1].tobytes()
