"""GPU: stereo rectification of raw pairs (orbx_rectifier_*, orbx_rectify_device, orbx_stereo_frame(_view)_rectified) against the
restatement in tests/rectify_ref.py: maps bit for bit, rectified images byte for byte, frames field for field against stereo_frame
on the numpy-rectified pair, and the rectified images' keypoints / descriptors against the CPU oracle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_ref as R   # noqa: E402
import rgbd_ref           # noqa: E402

pytestmark = pytest.mark.gpu
NF = 1200   # the EuRoC settings: 1200 features, 1.2, 8 levels, 20 / 7
MBF, MB = 47.90639384423901, 0.11007784219
EL, ER = R.EUROC_L, R.EUROC_R
I3 = np.eye(3)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def rot(axis, deg):
    t = np.radians(deg)
    c, s = np.cos(t), np.sin(t)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


TUM_D = [rgbd_ref.TUM1[k] for k in ("k1", "k2", "p1", "p2", "k3")]
RATIONAL_D = [0.12, -0.05, 0.0011, -0.0007, 0.01, 0.31, -0.02, 0.005]
# _w = j/64 - 2 exactly: zero at column 128 (NaN map values along that column)
P_W0 = np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0 / 128, 0, -0.5]])
# ir = diag(-1e40, 1e40, 1): u = -inf past column 0, v = +inf past row 0 as floats (finite doubles above FLT_MAX)
P_INF = np.array([[-1e-40, 0, 0], [0, 1e-40, 0], [0, 0, 1.0]])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_map_bits(got, ref, what=""):
    gn, rn = np.isnan(got), np.isnan(ref)
    np.testing.assert_array_equal(gn, rn, err_msg=what + " NaN positions")
    np.testing.assert_array_equal(bits(np.where(gn, 0, got)), bits(np.where(rn, 0, ref)), err_msg=what)


def tile_forms(mapx, mapy, budget=4096):
    """(tiles, gather tiles) of the 64 x 16 output tiles: a tile gathers when the bounding box of its taps with non-negative
    coordinates holds more than `budget` pixels."""
    sx, sy, _, _ = R.fixed_maps(mapx, mapy)
    h, w = mapx.shape
    n = g = 0
    for y0 in range(0, h, 16):
        for x0 in range(0, w, 64):
            a, b = sx[y0:y0 + 16, x0:x0 + 64], sy[y0:y0 + 16, x0:x0 + 64]
            ok = (a + 1 >= 0) & (b + 1 >= 0)
            n += 1
            if ok.any():
                fw = (a[ok] + 1).max() - np.maximum(a[ok], 0).min() + 1
                fh = (b[ok] + 1).max() - np.maximum(b[ok], 0).min() + 1
                g += int(fw * fh > budget)
    return n, g


MAP_CASES = {
    "euroc_752x480": (EL["K"], EL["D"], EL["R"], EL["P"], 752, 480),
    "euroc_right": (ER["K"], ER["D"], ER["R"], ER["P"], 752, 480),
    "kitti_1241x376": (EL["K"], EL["D"][:4] + [0.0], I3, EL["P"], 1241, 376),
    "vga_zero_D": (EL["K"], [0, 0, 0, 0], I3, EL["K"], 640, 480),
    "hd_1920x1080": (np.array(EL["K"]) * [[2.5, 1, 2.5], [1, 2.2, 2.2], [1, 1, 1]], EL["D"], rot("x", 2.0), EL["P"], 1920, 1080),
    "odd_333x221": (EL["K"], EL["D"], rot("z", -3.0), EL["P"], 333, 221),
    "tum_strong_k3": (EL["K"], TUM_D, rot("y", 4.0), EL["P"], 752, 480),
    "rational_8": (EL["K"], RATIONAL_D, rot("z", 1.5), EL["P"], 752, 480),
    "other_focal_centre": (EL["K"], EL["D"], I3, [[380.0, 0, 352.5, 0], [0, 395.0, 231.25, 0], [0, 0, 1, 0]], 752, 480),
    "rot_y80": (EL["K"], EL["D"], rot("y", 80.0), EL["P"], 752, 480),
    "w_crosses_zero": ([[400.0, 0, 300.0], [0, 400.0, 200.0], [0, 0, 1]], [0, 0, 0, 0], I3, P_W0, 320, 48),
    "inf_values": ([[400.0, 0, 300.0], [0, 400.0, 200.0], [0, 0, 1]], [0, 0, 0, 0], I3, P_INF, 320, 48),
}


def make(pkg, case):
    K, D, Rm, P, w, h = MAP_CASES[case]
    return pkg.StereoRectifier(K, D, Rm, P, w, h), R.init_rectify_map(K, D, Rm, P, w, h)


# ---- 1. maps bit for bit
@pytest.mark.parametrize("case", sorted(MAP_CASES))
def test_maps_bit_exact(pkg, case):
    r, (mx, my) = make(pkg, case)
    gx, gy = r.maps()
    assert_map_bits(gx, mx, case + " mapx")
    assert_map_bits(gy, my, case + " mapy")
    info = r.info()
    n, g = tile_forms(mx, my)
    assert info["tiles"] == n and info["gather_tiles"] == g, (info, n, g)
    assert info["device_bytes"] >= 16 * mx.size
    if case == "euroc_752x480":
        assert g == 0
    if case == "w_crosses_zero":
        assert np.isnan(mx).any() and np.isnan(my).any()
    if case == "inf_values":
        assert np.isneginf(mx).any() and np.isposinf(my).any()
    if case == "rot_y80":
        assert np.abs(mx).max() > 1e9 and 0 < g < n


def test_d_variants_differ(pkg):
    # 4 coefficients = 5 with k3 = 0; the k3 slot matters when set
    K = EL["K"]
    m4 = pkg.StereoRectifier(K, EL["D"], I3, EL["P"], 64, 32).maps()[0]
    m5 = pkg.StereoRectifier(K, EL["D"] + [0.0], I3, EL["P"], 64, 32).maps()[0]
    m5k = pkg.StereoRectifier(K, EL["D"] + [0.05], I3, EL["P"], 64, 32).maps()[0]
    assert (bits(m4) == bits(m5)).all() and not (bits(m4) == bits(m5k)).all()


# ---- 2. rectify_device byte for byte
def device_batch(torch, imgs, stride, image_stride):
    B = len(imgs)
    buf = np.zeros(B * image_stride + 64, np.uint8)
    for b, im in enumerate(imgs):
        h = im.shape[0]
        row = im.reshape(h, -1)
        for y in range(h):
            o = b * image_stride + y * stride
            buf[o:o + row.shape[1]] = row[y]
    return torch.from_numpy(buf).cuda()


def raw_images(synth, B, sw, sh, ch, k0=0):
    out = []
    for b in range(B):
        g = synth.frame(sw, sh, 11 + k0 + b).astype(np.int32)
        if ch == 1:
            out.append(g.astype(np.uint8))
        else:
            c = [g, (3 * g) // 4 + 40 + b % 7, 255 - g // 2] + ([np.full_like(g, 200 - b)] if ch == 4 else [])
            out.append(np.stack(c, -1).astype(np.uint8))
    return out


@pytest.mark.parametrize("ch,rgb,B,B0,cases,src,pad", [
    (1, 1, 1, 1, ("euroc_752x480", "euroc_right"), None, 0),
    (1, 0, 2, 1, ("euroc_752x480", "euroc_right"), None, 3),
    (3, 1, 5, 2, ("euroc_752x480", "euroc_right"), None, 1),
    (3, 0, 2, 1, ("euroc_752x480", "rot_y80"), (715, 499), 5),
    (4, 1, 5, 3, ("euroc_right", "euroc_752x480"), (793, 457), 2),
    (4, 0, 2, 0, ("euroc_752x480", "euroc_right"), None, 0),
    (1, 1, 3, 2, ("odd_333x221", "odd_333x221"), (200, 150), 7),       # tiles wholly outside the source
    (1, 0, 4, 2, ("rot_y80", "w_crosses_zero"), None, 1),              # (the second map's size differs: rejected below)
    (3, 1, 2, 1, ("rot_y80", "rot_y80"), None, 0),                     # LDS and gather tiles, huge map values
    (1, 1, 64, 32, ("euroc_752x480", "euroc_right"), None, 0),
])
def test_rectify_device_byte_exact(pkg, synth, torch, ch, rgb, B, B0, cases, src, pad):
    (r0, m0), (r1, m1) = make(pkg, cases[0]), make(pkg, cases[1])
    w, h = MAP_CASES[cases[0]][4:]
    sw, sh = src if src else (w, h)
    stride = sw * ch + pad
    image_stride = stride * sh + 3 * pad
    imgs = raw_images(synth, B, sw, sh, ch)
    d_src = device_batch(torch, imgs, stride, image_stride)
    gstride = w + (pad | 1) if pad else w
    gimg = gstride * h + pad
    d_out = torch.full((B * gimg + 64,), 77, dtype=torch.uint8, device="cuda")
    if MAP_CASES[cases[1]][4:] != (w, h):
        with pytest.raises(pkg.OrbxError) as e:
            pkg.rectify_device(r0, r1, B0, d_src.data_ptr(), B, sw, sh, ch, rgb, stride, image_stride, d_out.data_ptr(), gstride, gimg)
        assert e.value.status == pkg.ORBX_ERR_ARG
        return
    pkg.rectify_device(r0, r1, B0, d_src.data_ptr(), B, sw, sh, ch, rgb, stride, image_stride, d_out.data_ptr(), gstride, gimg)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    for b in range(B):
        mx, my = m0 if b < B0 else m1
        ref = R.rectify_gray(imgs[b], mx, my, rgb=bool(rgb))
        got = out[b * gimg:b * gimg + gstride * h].reshape(h, gstride)
        np.testing.assert_array_equal(got[:, :w], ref, err_msg="image %d" % b)
        assert (got[:, w:] == 77).all(), "row padding written"
    assert (out[B * gimg:] == 77).all()
    if src is None and ch == 1 and cases[0] == "euroc_752x480":
        assert ref.any()


@pytest.mark.parametrize("ch,rgb", [(1, 1), (3, 0), (4, 1)])
def test_nonfinite_map_values_read_nothing(pkg, synth, torch, ch, rgb):
    # images [0, 2) through the map whose _w crosses zero (NaN in both maps), [2, 4) through the one with -inf in x and +inf in y, in
    # one launch.  No source pixel is 0, so a NaN or inf that became an address inside the image (a GPU float -> int conversion gives
    # 0 for NaN) would show as a non-zero output where the map is not finite.
    (r0, m0), (r1, m1) = make(pkg, "w_crosses_zero"), make(pkg, "inf_values")
    w, h = MAP_CASES["w_crosses_zero"][4:]
    assert MAP_CASES["inf_values"][4:] == (w, h)
    sw, sh, B, B0 = 640, 480, 4, 2
    stride = sw * ch + 3
    image_stride = stride * sh + 5
    imgs = [np.maximum(im, 1) for im in raw_images(synth, B, sw, sh, ch, k0=40)]
    d_src = device_batch(torch, imgs, stride, image_stride)
    gstride, gimg = w + 3, (w + 3) * h + 1
    d_out = torch.full((B * gimg + 64,), 77, dtype=torch.uint8, device="cuda")
    pkg.rectify_device(r0, r1, B0, d_src.data_ptr(), B, sw, sh, ch, rgb, stride, image_stride, d_out.data_ptr(), gstride, gimg)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.isnan(m0[0]).any() and np.isnan(m0[1]).any() and np.isneginf(m1[0]).any() and np.isposinf(m1[1]).any()
    for b in range(B):
        mx, my = m0 if b < B0 else m1
        bad = ~(np.isfinite(mx) & np.isfinite(my))
        sx, sy, _, _ = R.fixed_maps(mx, my)
        reads = ~bad & (sx + 1 >= 0) & (sx < sw) & (sy + 1 >= 0) & (sy < sh)   # finite pixels with a tap inside the image
        assert bad.sum() >= 48 and reads.any()
        ref = R.rectify_gray(imgs[b], mx, my, rgb=bool(rgb))
        got = out[b * gimg:b * gimg + gstride * h].reshape(h, gstride)
        np.testing.assert_array_equal(got[:, :w], ref, err_msg="image %d" % b)
        assert (got[:, :w][bad] == 0).all(), "image %d: a pixel whose map value is not finite read the image" % b
        assert (got[:, :w][reads] > 0).any(), "image %d" % b
        assert (got[:, w:] == 77).all(), "row padding written"
    assert (out[B * gimg:] == 77).all()


# ---- 3. one frame: stereo_frame_rectified(raw) == stereo_frame(numpy-rectified)
def colour_pair(l, r):
    def col(g, k):
        g = g.astype(np.int32)
        return np.stack([g, (3 * g) // 4 + 40 + k, 255 - g // 2], -1).astype(np.uint8)
    return col(l, 0), col(r, 3)


def assert_frames_equal(a, b, what=""):
    for f in ("kl", "dl", "kr", "dr", "uright", "depth"):
        assert np.asarray(a[f]).tobytes() == np.asarray(b[f]).tobytes(), what + f
    assert a["nmatch"] == b["nmatch"], what


def assert_kp_equal(got, ref, what=""):
    assert len(got) == len(ref), what
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        np.testing.assert_array_equal(got[f], ref[f], err_msg=what + f)
    np.testing.assert_allclose(got["angle"], ref["angle"], atol=1e-4, rtol=0, err_msg=what + "angle")


@pytest.mark.parametrize("ch", [1, 3])
def test_stereo_frame_rectified_equals_stereo_frame_on_rectified_pair(pkg, synth, oracle, ch):
    w, h = R.EUROC_SIZE
    (rl, ml), (rr, mr) = make(pkg, "euroc_752x480"), make(pkg, "euroc_right")
    left, right = synth.stereo_pair_blocky(w, h, 7)
    if ch == 3:
        left, right = colour_pair(left, right)
    gl, gr = R.rectify_gray(left, *ml, rgb=False), R.rectify_gray(right, *mr, rgb=False)
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    got = ex.stereo_frame_rectified(rl, rr, left, right, MBF, MB, rgb=False)
    ref = pkg.ORBextractor(NF, 1.2, 8, 20, 7).stereo_frame(gl, gr, MBF, MB)
    assert len(got["kl"]) > 200 and got["nmatch"] > 5
    assert_frames_equal(got, ref, "ch%d " % ch)
    okl, odl = oracle.Extractor(NF, 1.2, 8, 20, 7).extract(gl)
    okr, odr = oracle.Extractor(NF, 1.2, 8, 20, 7).extract(gr)
    assert_kp_equal(got["kl"], okl, "left ")
    assert_kp_equal(got["kr"], okr, "right ")
    assert (got["dl"] == odl).all() and (got["dr"] == odr).all()


def test_identity_maps_equal_stereo_frame_on_raw(pkg, synth):
    w, h = 640, 480
    K = [[450.0, 0, 320.0], [0, 450.0, 240.0], [0, 0, 1]]
    rl, rr = pkg.StereoRectifier(K, [0, 0, 0, 0], I3, K, w, h), pkg.StereoRectifier(K, [0, 0, 0, 0, 0], I3, K, w, h)
    left, right = synth.stereo_pair_blocky(w, h, 3)
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    a = ex.stereo_frame_rectified(rl, rr, left, right, MBF, MB)
    b = pkg.ORBextractor(NF, 1.2, 8, 20, 7).stereo_frame(left, right, MBF, MB)
    assert_frames_equal(a, b)


# ---- 4. the latency form: pinned, device and pageable inputs; three calls in a row keep the previous record
@pytest.mark.parametrize("kind", ["pageable", "pinned", "device"])
def test_view_rectified_equals_host_form(pkg, synth, torch, kind):
    w, h = R.EUROC_SIZE
    rl, rr = make(pkg, "euroc_752x480")[0], make(pkg, "euroc_right")[0]
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    host = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    frames = []
    for k in range(3):
        l, r = synth.stereo_pair_blocky(w, h, 20 + k)
        if k == 1:
            l, r = colour_pair(l, r)
        frames.append((l, r))
    refs = [host.stereo_frame_rectified(rl, rr, l, r, MBF, MB, rgb=True) for l, r in frames]
    prev = None
    for k, (l, r) in enumerate(frames):
        if kind == "pageable":
            a, b = l, r
        else:
            a, b = torch.from_numpy(l), torch.from_numpy(r)
            a, b = (a.pin_memory(), b.pin_memory()) if kind == "pinned" else (a.cuda(), b.cuda())
        got = ex.stereo_frame_view_rectified(rl, rr, a, b, MBF, MB, rgb=True)
        assert_frames_equal(got, refs[k], "%s call %d " % (kind, k))
        if prev is not None:   # the previous call's record is still intact
            assert_frames_equal(prev[0], refs[prev[1]], "%s previous of call %d " % (kind, k))
        prev = (got, k)
        if kind != "pageable":
            torch.cuda.synchronize()


def test_empty_images_and_argument_errors(pkg, synth):
    w, h = 320, 240
    K = [[250.0, 0, 160.0], [0, 250.0, 120.0], [0, 0, 1]]
    rl = pkg.StereoRectifier(K, [0, 0, 0, 0], I3, K, w, h)
    rbig = pkg.StereoRectifier(K, [0, 0, 0, 0], I3, K, w + 1, h)
    img = np.zeros((h, w), np.uint8)
    ex = pkg.ORBextractor(500, 1.2, 8, 20, 7)
    L = pkg.lib()

    def status(fn, *a):
        with pytest.raises(pkg.OrbxError) as e:
            fn(*a)
        return e.value.status
    A = pkg.ORBX_ERR_ARG
    # creation: coefficient counts, singular Ar*R, sizes
    for n in (0, 3, 6, 7, 12, 14):
        assert status(pkg.StereoRectifier, K, np.zeros(n), I3, K, w, h) == A, n
    assert status(pkg.StereoRectifier, K, [0, 0, 0, 0], np.zeros((3, 3)), K, w, h) == A
    assert status(pkg.StereoRectifier, K, [0, 0, 0, 0], I3, [[1, 2, 3], [2, 4, 6], [0, 0, 1]], w, h) == A
    for ww, hh in ((0, h), (w, 0), (4096, h), (w, 4096)):
        assert status(pkg.StereoRectifier, K, [0, 0, 0, 0], I3, K, ww, hh) == A
    # frames: NULL rectifier, channels, map size, stride
    assert status(ex.stereo_frame_rectified, None, rl, img, img, MBF, MB) == A
    assert status(ex.stereo_frame_rectified, rl, rbig, img, img, MBF, MB) == A
    assert status(ex.stereo_frame_view_rectified, rl, None, img, img, MBF, MB) == A
    assert status(ex.stereo_frame_view_rectified, rl, rl, img, img, MBF, MB, True, None, 2) == A
    assert status(ex.stereo_frame_view_rectified, rl, rl, img, img, MBF, MB, True, None, 1, w - 1) == A
    v = pkg.StereoView()
    p = img.ctypes.data
    img3 = np.zeros((h, w, 3), np.uint8)
    p3 = img3.ctypes.data
    assert L.orbx_stereo_frame_view_rectified(ex._h, rl.handle, rl.handle, p3, p3, 3, 1, w, h, w * 3 - 1, MBF, MB, C.byref(v)) == A
    assert L.orbx_stereo_frame_view_rectified(ex._h, rl.handle, rl.handle, p3, p3, 3, 1, w, h, w * 3, MBF, MB, C.byref(v)) == pkg.ORBX_OK
    # empty image: OK, zero counts
    e = ex.stereo_frame_rectified(rl, rl, np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.uint8), MBF, MB)
    assert len(e["kl"]) == 0 and e["nmatch"] == 0
    assert L.orbx_stereo_frame_view_rectified(ex._h, rl.handle, rl.handle, None, None, 1, 1, 0, 0, 0, MBF, MB, C.byref(v)) == pkg.ORBX_OK
    assert v.nl == 0 and v.nr == 0
    # rectify_device: NULL rectifier for used images, channels, strides, map sizes that differ
    d = pkg.lib()
    assert d.orbx_rectify_device(None, rl.handle, 1, p, 2, w, h, 1, 1, w, w * h, p, w, w * h, None) == A
    assert d.orbx_rectify_device(rl.handle, rl.handle, 1, p, 2, w, h, 2, 1, w, w * h, p, w, w * h, None) == A
    assert d.orbx_rectify_device(rl.handle, rl.handle, 1, p, 2, w, h, 1, 1, w - 1, w * h, p, w, w * h, None) == A
    assert d.orbx_rectify_device(rl.handle, rbig.handle, 1, p, 2, w, h, 1, 1, w, w * h, p, w, w * h, None) == A
    assert d.orbx_rectifier_info(None, None, None, None) == A and d.orbx_rectifier_maps(None, None, None) == A
