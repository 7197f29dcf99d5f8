"""GPU: the RGB-D front end (orbx_gray_from_color_device, orbm_rgbd_batch_device, orbx_rgbd_frame) of the product library against
the restatement in tests/rgbd_ref.py and the CPU oracle's extraction of the restated gray image: colour conversion byte for byte,
mvKeysUn / mvuRight / mvDepth bit for bit, keypoints and descriptors as every extraction test demands."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgbd_ref as R          # noqa: E402
import tracking_chain as tc   # noqa: E402

pytestmark = pytest.mark.gpu
NF = 1000   # config/Asus.yaml: 1000 features, 1.2, 8 levels, 20 / 7
K1_ZERO = dict(R.TUM1, k1=0.0)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def colorize(g, channels, k=0):
    """A colour image whose restated gray keeps the corners of g (every channel monotone in g)."""
    g = g.astype(np.int32)
    ch = [g, (3 * g) // 4 + 40 + (k % 7), 255 - g // 2]
    if channels == 4:
        ch.append(np.full_like(g, 200))
    return np.stack(ch, -1).astype(np.uint8)


def depth_image(w, h, kind, k=0):
    """kind u16: millimetres * 5 (DepthMapFactor 5000) with zero holes; f32: metres with NaN / 0 / negative / +-inf holes."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    metres = 1.0 + 1.5 * x / w + 0.7 * y / h + 0.05 * np.sin(x * 0.37 + y * 0.11 + k)
    hole = ((x.astype(int) * 7 + y.astype(int) * 13) % 5) == 0
    if kind == "u16":
        d = np.round(metres * 5000).astype(np.uint16)
        d[hole] = 0
        return d, 1.0 / 5000
    d = metres.astype(np.float32)
    sel = (x.astype(int) + y.astype(int)) % 5
    for s, v in enumerate((np.nan, 0.0, -1.5, np.inf, -np.inf)):
        d[hole & (sel == s)] = v
    return d, 1.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_kp_equal(got, ref, what=""):
    assert len(got) == len(ref), what
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        np.testing.assert_array_equal(got[f], ref[f], err_msg=what + f)
    np.testing.assert_allclose(got["angle"], ref["angle"], atol=1e-4, rtol=0, err_msg=what + "angle")


def assert_assoc_bits(kun, ur, dp, kp, depth, factor, cam, what=""):
    rk, rur, rdp = R.rgbd_assoc(kp, depth, factor, cam)
    np.testing.assert_array_equal(bits(kun["x"]), bits(rk["x"]), err_msg=what + "kun.x")
    np.testing.assert_array_equal(bits(kun["y"]), bits(rk["y"]), err_msg=what + "kun.y")
    for f in ("size", "angle", "response", "octave", "class_id"):
        np.testing.assert_array_equal(kun[f], kp[f], err_msg=what + f)
    np.testing.assert_array_equal(bits(ur), bits(rur), err_msg=what + "uright")
    np.testing.assert_array_equal(bits(dp), bits(rdp), err_msg=what + "depth")


# ---- 1. colour conversion: every colour, both orders, 3 and 4 channels; odd widths, padded strides, unaligned rows
@pytest.mark.parametrize("channels", [3, 4])
def test_every_colour_byte_exact(pkg, torch, channels):
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    img = np.stack([v & 255, (v >> 8) & 255, v >> 16] + ([255 - (v & 255)] if channels == 4 else []), -1).astype(np.uint8)
    d = torch.from_numpy(img).cuda()
    out = torch.zeros((4096, 4096), dtype=torch.uint8, device="cuda")
    for rgb in (True, False):
        pkg.gray_from_color_device(d.data_ptr(), 1, 4096, 4096, channels, rgb, 4096 * channels, 0, out.data_ptr(), 4096, 0)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(out.cpu().numpy(), R.gray_from_color(img, rgb))


@pytest.mark.parametrize("w,h,B,pad,offset", [(321, 7, 3, 5, 0), (640, 4, 2, 0, 1), (1, 3, 1, 3, 0), (1243, 5, 4, 16, 3), (7, 9, 5, 1, 2)])
@pytest.mark.parametrize("channels", [3, 4])
def test_odd_widths_and_strides(pkg, torch, w, h, B, pad, offset, channels):
    rng = np.random.default_rng(w * 31 + h + channels)
    stride = w * channels + pad
    istride = stride * h + 11
    buf = rng.integers(0, 256, offset + istride * B, dtype=np.uint8)
    d = torch.from_numpy(buf).cuda()
    gstride, gistride = w + 3, (w + 3) * h + 5
    sentinel = 0x5A
    out = torch.full((gistride * B + 8,), sentinel, dtype=torch.uint8, device="cuda")
    for rgb in (True, False):
        pkg.gray_from_color_device(d.data_ptr() + offset, B, w, h, channels, rgb, stride, istride, out.data_ptr(), gstride, gistride)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        written = np.zeros(o.shape, bool)
        for b in range(B):
            rows = np.stack([buf[offset + b * istride + y * stride: offset + b * istride + y * stride + w * channels] for y in range(h)])
            ref = R.gray_from_color(rows.reshape(h, w, channels), rgb)
            for y in range(h):
                s = b * gistride + y * gstride
                np.testing.assert_array_equal(o[s:s + w], ref[y], err_msg="image %d row %d" % (b, y))
                written[s:s + w] = True
        assert (o[~written] == sentinel).all(), "bytes outside the gray images were written"


# ---- 2. one frame host to host against the oracle + restatement
@pytest.mark.parametrize("w,h", [(640, 480), (752, 480), (321, 241)])
@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("dist", ["none", "tum1", "k1_zero"])
def test_rgbd_frame(pkg, synth, oracle, w, h, kind, dist):
    cam = {"none": R.ASUS, "tum1": R.TUM1, "k1_zero": K1_ZERO}[dist]
    k = w + h + len(kind) + len(dist)
    channels, rgb = (3, True) if k % 3 == 0 else (4, False) if k % 3 == 1 else (3, False)
    color = colorize(synth.frame(w, h, k), channels, k)
    depth, factor = depth_image(w, h, kind, k)
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    r = ex.rgbd_frame(color, depth, pkg.RGBDCamera(**cam), factor, rgb=rgb)
    gray = R.gray_from_color(color, rgb)
    ok, od = oracle.Extractor(NF, 1.2, 8, 20, 7).extract(gray)
    assert len(ok) > 100
    assert_kp_equal(r["kp"], ok)
    np.testing.assert_array_equal(r["desc"], od)
    assert_assoc_bits(r["kun"], r["uright"], r["depth"], r["kp"], depth, factor, cam)
    if dist != "tum1":
        assert r["kun"].tobytes() == r["kp"].tobytes()
    else:
        assert (r["kun"]["x"] != r["kp"]["x"]).mean() > 0.9
    has = r["depth"] > 0
    assert 0.5 < has.mean() < 0.95, has.mean()   # both branches are exercised
    # again on the same handle: the scratch is reused, the results do not change
    r2 = ex.rgbd_frame(color, depth, pkg.RGBDCamera(**cam), factor, rgb=rgb)
    for f in r:
        assert r2[f].tobytes() == r[f].tobytes(), f
    ex.close()


def test_gray_input_and_row_strided_views(pkg, synth, oracle):
    """channels 1 (what Tracking already converted) and row-strided colour / depth views (ROIs of wider images)."""
    w, h = 640, 480
    big = colorize(synth.frame(w + 40, h, 3), 3)
    color = big[:, 20:20 + w]
    dbig, factor = depth_image(w + 40, h, "f32", 3)
    depth = dbig[:, 20:20 + w]
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    r = ex.rgbd_frame(color, depth, pkg.RGBDCamera(**R.TUM1), factor, rgb=True)
    gray = R.gray_from_color(np.ascontiguousarray(color), True)
    rg = ex.rgbd_frame(gray, np.ascontiguousarray(depth), pkg.RGBDCamera(**R.TUM1), factor)
    for f in r:
        assert rg[f].tobytes() == r[f].tobytes(), f
    ok, od = oracle.Extractor(NF, 1.2, 8, 20, 7).extract(gray)
    assert_kp_equal(r["kp"], ok)
    np.testing.assert_array_equal(r["desc"], od)
    assert_assoc_bits(r["kun"], r["uright"], r["depth"], r["kp"], np.ascontiguousarray(depth), factor, R.TUM1)


# ---- 3. monocular tail
@pytest.mark.parametrize("dist", ["none", "tum1"])
def test_monocular_tail(pkg, synth, oracle, dist):
    cam = R.TUM1 if dist == "tum1" else R.ASUS
    w, h = 752, 480
    color = colorize(synth.frame(w, h, 9), 3)
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    r = ex.rgbd_frame(color, None, pkg.RGBDCamera(**cam), 1.0)
    assert len(r["kp"]) > 100
    assert (r["uright"] == -1).all() and (r["depth"] == -1).all()
    assert_assoc_bits(r["kun"], r["uright"], r["depth"], r["kp"], None, 1.0, cam)


# ---- 4. the batched form: each frame equals rgbd_frame of that frame; rows past the count untouched
@pytest.mark.parametrize("B", [1, 5, 64])
def test_batch_device_equals_frame(pkg, synth, torch, B):
    w, h, cam = 640, 480, R.TUM1
    colors, depths = [], []
    for b in range(B):
        g = synth.frame(w, h, 40 + b % 9)
        if b % 3 == 1:
            g[:, : w * (b % 5 + 1) // 7] = 128   # flat regions: uneven keypoint counts
        colors.append(colorize(g, 4, b))
        depths.append(depth_image(w, h, "u16", b)[0])
    factor = 1.0 / 5000
    colors, depths = np.stack(colors), np.stack(depths)
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    ex(np.zeros((h, w), np.uint8) + 90)
    cap = ex.max_keypoints() + 64
    d_col = torch.from_numpy(colors).cuda()
    d_dep = torch.from_numpy(depths).cuda()
    gs = w + 64
    d_gray = torch.zeros((B, h, gs), dtype=torch.uint8, device="cuda")
    kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    kun = torch.full((B, cap, 7), 12345.0, dtype=torch.float32, device="cuda")
    ur = torch.full((B, cap), 12345.0, dtype=torch.float32, device="cuda")
    dp = torch.full((B, cap), 12345.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    pkg.gray_from_color_device(d_col.data_ptr(), B, w, h, 4, False, w * 4, w * h * 4, d_gray.data_ptr(), gs, gs * h, st)
    ex.extract_batch_device(d_gray.data_ptr(), B, w, h, gs, gs * h, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), cap, st)
    pkg.rgbd_batch_device(kps.data_ptr(), cnt.data_ptr(), B, cap, d_dep.data_ptr(), pkg.DEPTH_U16, w, h, w * 2, w * h * 2, factor,
                          pkg.RGBDCamera(**cam), kun.data_ptr(), ur.data_ptr(), dp.data_ptr(), st)
    torch.cuda.synchronize()
    n = cnt.cpu().numpy()
    if B > 1:
        assert len(set(n.tolist())) > 1, n
    g_kps = kps.cpu().numpy().view(pkg.KP_DTYPE).reshape(B, cap)
    g_desc, g_kun = desc.cpu().numpy(), kun.cpu().numpy().view(pkg.KP_DTYPE).reshape(B, cap)
    g_ur, g_dp = ur.cpu().numpy(), dp.cpu().numpy()
    np.testing.assert_array_equal(d_gray.cpu().numpy()[:, :, :w], R.gray_from_color(colors, False))
    ex1 = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    for b in range(B):
        r = ex1.rgbd_frame(colors[b], depths[b], pkg.RGBDCamera(**cam), factor, rgb=False)
        m = n[b]
        assert m == len(r["kp"]), b
        assert g_kps[b, :m].tobytes() == r["kp"].tobytes(), b
        assert g_desc[b, :m].tobytes() == r["desc"].tobytes(), b
        assert g_kun[b, :m].tobytes() == r["kun"].tobytes(), b
        assert g_ur[b, :m].tobytes() == r["uright"].tobytes() and g_dp[b, :m].tobytes() == r["depth"].tobytes(), b
        assert (g_ur[b, m:] == 12345.0).all() and (g_dp[b, m:] == 12345.0).all(), b
        assert (g_kun[b, m:].view(np.float32).reshape(-1, 7)[:, :5] == 12345.0).all(), b
    # the monocular tail on the same device arrays
    pkg.rgbd_batch_device(kps.data_ptr(), cnt.data_ptr(), B, cap, None, 0, w, h, 0, 0, 1.0, pkg.RGBDCamera(**cam), kun.data_ptr(),
                          ur.data_ptr(), dp.data_ptr(), st)
    torch.cuda.synchronize()
    g_ur, g_dp = ur.cpu().numpy(), dp.cpu().numpy()
    for b in range(B):
        assert (g_ur[b, :n[b]] == -1).all() and (g_dp[b, :n[b]] == -1).all() and (g_ur[b, n[b]:] == 12345.0).all()


# ---- 5. argument errors and the capacity clamp
def test_argument_errors_and_capacity(pkg, synth):
    w, h = 640, 480
    color = colorize(synth.frame(w, h, 5), 3)
    depth, factor = depth_image(w, h, "u16")
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    L, cam = ex._L, pkg.RGBDCamera(**R.TUM1)
    cap = 4000
    kp, kun = np.zeros(cap, pkg.KP_DTYPE), np.zeros(cap, pkg.KP_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    ur, dp = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    n = C.c_int(-7)
    p = pkg._p

    def call(img=color, ch=3, dep=depth, dtype=pkg.DEPTH_U16, c=cam, cp=cap, ww=w, hh=h, stride=w * 3):
        n.value = -7
        return L.orbx_rgbd_frame(ex._h, p(img), ch, 1, ww, hh, stride, p(dep), dtype, w * 2, factor, None if c is None else C.byref(c), cp,
                                 p(kp), p(desc), C.byref(n), p(kun), p(ur), p(dp))
    assert call(ch=2) == pkg.ORBX_ERR_ARG
    assert call(dtype=7) == pkg.ORBX_ERR_ARG
    assert call(c=None) == pkg.ORBX_ERR_ARG
    assert call(stride=w * 3 - 1) == pkg.ORBX_ERR_ARG
    assert call(cp=0) == pkg.ORBX_ERR_ARG
    assert call(ww=0) == pkg.ORBX_OK and n.value == 0
    assert call(img=None) == pkg.ORBX_OK and n.value == 0
    assert call() == pkg.ORBX_OK
    full = n.value
    ref = [a[:full].copy() for a in (kp, desc, kun, ur, dp)]
    assert full > 100
    for a in (kp, desc, kun, ur, dp):
        a[...] = 0
    assert call(cp=50) == pkg.ORBX_ERR_CAPACITY and n.value == 50
    for a, r in zip((kp, desc, kun, ur, dp), ref):
        assert a[:50].tobytes() == r[:50].tobytes()
        assert not np.frombuffer(a[50:].tobytes(), np.uint8).any(), "rows past the capacity were written"
    # the batched entry points
    d = L.orbm_rgbd_batch_device
    assert d(None, None, 1, 16, None, 0, w, h, 0, 0, 1.0, C.byref(cam), None, None, None, None) == pkg.ORBX_ERR_ARG
    assert L.orbx_gray_from_color_device(None, 1, w, h, 3, 1, w * 3, 0, None, w, 0, None) == pkg.ORBX_ERR_ARG
    with pytest.raises(pkg.OrbxError):
        pkg.gray_from_color_device(16, 1, w, h, 2, True, w * 3, 0, 16, w, 0)


# ---- 6. two distorted RGB-D frames through the device-resident SearchByProjection(cur, last)
def test_search_by_projection_on_rgbd_device_outputs(pkg, synth, oracle, torch):
    w, h, cam = 640, 480, R.TUM1
    base = synth.frame(w + 16, h, 77)
    shift = 4
    frames = [base[:, 8:8 + w], base[:, 8 - shift:8 - shift + w]]    # the camera moves by tx: the scene moves by +shift px
    Z = 2.0
    ys, xs = np.mgrid[0:h, 0:w]
    depth = (np.float32(Z) + np.float32(0.02) * np.sin(xs * 0.05 + ys * 0.03)).astype(np.float32)
    colors = np.stack([colorize(np.ascontiguousarray(f), 3) for f in frames])
    ex = pkg.ORBextractor(NF, 1.2, 8, 20, 7)
    ex(np.zeros((h, w), np.uint8) + 90)
    cap = ex.max_keypoints() + 64
    B = 2
    d_col = torch.from_numpy(colors).cuda()
    d_dep = torch.from_numpy(np.stack([depth, depth])).cuda()
    d_gray = torch.zeros((B, h, w), dtype=torch.uint8, device="cuda")
    kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    kun = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    ur = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    dp = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    rcam = pkg.RGBDCamera(**cam)
    pkg.gray_from_color_device(d_col.data_ptr(), B, w, h, 3, True, w * 3, w * h * 3, d_gray.data_ptr(), w, w * h, st)
    ex.extract_batch_device(d_gray.data_ptr(), B, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), cap, st)
    pkg.rgbd_batch_device(kps.data_ptr(), cnt.data_ptr(), B, cap, d_dep.data_ptr(), pkg.DEPTH_F32, w, h, w * 4, w * h * 4, 1.0, rcam,
                          kun.data_ptr(), ur.data_ptr(), dp.data_ptr(), st)
    torch.cuda.synchronize()
    n = cnt.cpu().numpy()
    K = [kun.cpu().numpy().view(pkg.KP_DTYPE).reshape(B, cap)[b, :n[b]].copy() for b in range(B)]
    D = [desc.cpu().numpy()[b, :n[b]].copy() for b in range(B)]
    UR = [ur.cpu().numpy()[b, :n[b]].copy() for b in range(B)]
    DP = [dp.cpu().numpy()[b, :n[b]].copy() for b in range(B)]
    for b in range(B):
        kp = kps.cpu().numpy().view(pkg.KP_DTYPE).reshape(B, cap)[b, :n[b]]
        assert_assoc_bits(K[b], UR[b], DP[b], kp, depth, 1.0, cam, "frame %d " % b)
    # map points of the last frame: Frame::UnprojectStereo of its undistorted keypoints (src/Frame.cc:681-694), in a MapStore
    fx, fy, cx, cy = (np.float32(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    k0, z0 = K[0], DP[0]
    good = np.nonzero(z0 > 0)[0]
    X = ((k0["x"][good] - cx) * z0[good] / fx).astype(np.float32)
    Y = ((k0["y"][good] - cy) * z0[good] / fy).astype(np.float32)
    store = tc.MapStore()
    ids = store.add(np.stack([X, Y, z0[good]], 1), D[0][good], np.tile([0, 0, 1], (len(good), 1)), z0[good] * 1.5, z0[good] * 0.5, 2, False)
    last = np.zeros(n[0], pkg.LASTPT_DTYPE)
    last["has_mp"][good] = 1
    last["wx"][good], last["wy"][good], last["wz"][good] = store.pos[ids, 0], store.pos[ids, 1], store.pos[ids, 2]
    last["observations"][good] = store.obs[ids]
    kp0 = kps.cpu().numpy().view(pkg.KP_DTYPE).reshape(B, cap)[0, :n[0]]
    last["octave"], last["angle"] = kp0["octave"], K[0]["angle"]
    Tl = np.eye(4, dtype=np.float32)
    Tc = np.eye(4, dtype=np.float32)
    Tc[0, 3] = np.float32(shift * Z / float(fx))                        # the scene moves right: the camera moved left
    x0, x1, y0, y1 = R.compute_image_bounds(w, h, cam)
    geom, ogeom = pkg.GridGeom(), oracle.GridGeom()
    for g in (geom, ogeom):
        g.min_x, g.max_x, g.min_y, g.max_y = x0, x1, y0, y1
        g.inv_w = np.float32(64) / np.float32(x1 - x0)                   # FRAME_GRID_COLS / (mnMaxX - mnMinX) (src/Frame.cc:97-98)
        g.inv_h = np.float32(48) / np.float32(y1 - y0)
    mb = float(np.float32(cam["mbf"]) / fx)
    pcam = pkg.Camera(fx, fy, cx, cy, cam["mbf"], mb)
    ocam = oracle.Cam(fx, fy, cx, cy, cam["mbf"], mb)
    sf = ex.GetScaleFactors()
    d1 = desc[1].data_ptr()
    nm, cur = pkg.search_by_projection_frame_device(kun[1].data_ptr(), d1, ur[1].data_ptr(), int(n[1]), geom, sf, pcam, Tc, Tl, last,
                                                    desc[0].data_ptr(), np.full(n[1], -1, np.int32), None, 7.0, False, True, 0, st)
    onm, ocur = oracle.search_by_projection_frame(K[1], D[1], UR[1], ogeom, sf, ocam, Tc, Tl, last, D[0], np.full(n[1], -1, np.int32),
                                                  None, 7.0, False, True)
    assert nm == onm and (cur == ocur).all()
    assert nm > 50, nm
