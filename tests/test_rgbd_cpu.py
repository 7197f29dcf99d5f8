"""CPU: the numpy restatement of the reference's RGB-D front end (tests/rgbd_ref.py) against hand-derived values, the RGB-D entry
points in the library's exports, and their loud failure without a GPU."""
import ctypes as C

import numpy as np
import pytest

import rgbd_ref as R


def test_gray_of_primaries():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0]]], np.uint8)
    # (255*4899 + 8192) >> 14 = 76, (255*9617 + 8192) >> 14 = 150, (255*1868 + 8192) >> 14 = 29; the weights add up to 2^14
    np.testing.assert_array_equal(R.gray_from_color(px, rgb=True)[0], [76, 150, 29, 255, 0])
    np.testing.assert_array_equal(R.gray_from_color(px, rgb=False)[0], [29, 150, 76, 255, 0])
    rgba = np.concatenate([px, np.full(px.shape[:2] + (1,), 7, np.uint8)], axis=2)   # alpha is ignored
    np.testing.assert_array_equal(R.gray_from_color(rgba, rgb=True), R.gray_from_color(px, rgb=True))


def test_k1_zero_is_a_no_op_even_with_tangential_terms():
    kp = np.zeros(3, [("x", "<f4"), ("y", "<f4")])
    kp["x"], kp["y"] = [10.5, 300.25, 620.0], [5.0, 240.75, 470.5]
    cam = dict(R.TUM1, k1=0.0)   # p1, p2, k2, k3 != 0: the reference still copies mvKeys (src/Frame.cc:421-425)
    kun = R.undistort_keypoints(kp, cam)
    assert kun.tobytes() == kp.tobytes()
    moved = R.undistort_keypoints(kp, R.TUM1)
    assert (moved["x"] != kp["x"]).all()


@pytest.mark.parametrize("d", [np.nan, 0.0, -1.0, -np.inf])
def test_depth_holes_give_minus_one(d):
    kp = np.zeros(1, [("x", "<f4"), ("y", "<f4")])
    kp["x"], kp["y"] = 3.7, 1.2
    depth = np.full((4, 8), 2.0, np.float32)
    depth[1, 3] = d
    _, ur, dp = R.rgbd_assoc(kp, depth, 1.0, R.ASUS)
    assert ur[0] == -1 and dp[0] == -1
    depth[1, 3] = 2.0   # the sample is at (int(y), int(x)) = (1, 3)
    _, ur, dp = R.rgbd_assoc(kp, depth, 1.0, R.ASUS)
    assert dp[0] == 2.0 and ur[0] == np.float32(np.float32(3.7) - np.float32(40.0) / np.float32(2.0))


def test_depth_factor_rule():
    f32 = np.full((1, 1), 3.0, np.float32)
    assert not R.depth_converts(np.float32, 1.0) and R.depth_sample(f32, 0, 0, 1.0) == 3.0
    # |1.00002f - 1| = 2.0027e-5 > 1e-5: converted; 1 + 5e-6 is not
    assert R.depth_converts(np.float32, 1 + 2e-5)
    assert R.depth_sample(f32, 0, 0, 1 + 2e-5) == np.float32(3.0) * np.float32(1 + 2e-5) != 3.0
    assert not R.depth_converts(np.float32, 1 + 5e-6) and R.depth_sample(f32, 0, 0, 1 + 5e-6) == 3.0
    # CV_16U is always converted, also with factor 1; 1/5000 (TUM's DepthMapFactor 5000)
    u16 = np.array([[5000, 1]], np.uint16)
    assert R.depth_converts(np.uint16, 1.0) and R.depth_sample(u16, 1, 0, 1.0) == 1.0
    d = R.depth_sample(u16, 0, 0, 1 / 5000)
    assert d.dtype == np.float32 and d == np.float32(5000) * np.float32(1 / 5000) and abs(d - 1) < 1e-6


def test_undistortion_round_trip_tum_fr1():
    """The forward model then the restated cvUndistortPoints gives the points back within 1e-3 px wherever a keypoint of a
    640x480 image can lie 40 px or more inside the border (OpenCV's fixed five iterations do not converge that far in the very
    corners of this strong lens)."""
    xs, ys = np.meshgrid(np.linspace(0, 640, 81), np.linspace(0, 480, 61))
    xs, ys = xs.ravel(), ys.ravel()
    xd, yd = R.distort_points(xs, ys, R.TUM1)
    m = (xd >= 40) & (xd < 600) & (yd >= 40) & (yd < 440)
    assert m.sum() > 2000
    xu, yu = R.undistort_points(xd[m].astype(np.float32), yd[m].astype(np.float32), R.TUM1)
    assert xu.dtype == np.float32
    assert np.hypot(xu - xs[m], yu - ys[m]).max() < 1e-3


def test_image_bounds():
    assert R.compute_image_bounds(640, 480, R.ASUS) == (0, 640, 0, 480)
    x0, x1, y0, y1 = R.compute_image_bounds(640, 480, R.TUM1)
    assert 0 < x0 < 20 and 620 < x1 < 640 and 0 < y0 < 20 and 460 < y1 < 480


def test_rgbd_exports(pkg):
    for name in ("orbx_gray_from_color_device", "orbm_rgbd_batch_device", "orbx_rgbd_frame"):
        assert name in pkg.EXPORTS and hasattr(pkg.lib(), name)
    assert C.sizeof(pkg.RGBDCamera) == 40 and (pkg.DEPTH_U16, pkg.DEPTH_F32) == (2, 5)


def test_rgbd_without_gpu_fails_loudly(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible here")
    L = pkg.lib()
    cam = pkg.RGBDCamera(**R.ASUS)
    # (non-NULL placeholders: the calls stop at the device check, before anything is launched)
    rc = L.orbx_gray_from_color_device(64, 1, 8, 8, 3, 1, 24, 0, 64, 8, 0, None)
    assert rc == pkg.ORBX_ERR_NO_DEVICE, rc
    rc = L.orbm_rgbd_batch_device(64, 64, 1, 16, None, pkg.DEPTH_F32, 8, 8, 32, 0, 1.0, C.byref(cam), 64, 64, 64, None)
    assert rc == pkg.ORBX_ERR_NO_DEVICE, rc
    assert L.orbm_rgbd_batch_device(64, 64, 1, 16, None, 0, 8, 8, 32, 0, 1.0, None, 64, 64, 64, None) == pkg.ORBX_ERR_ARG
    with pytest.raises(pkg.OrbxError) as e:
        pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    assert e.value.status == pkg.ORBX_ERR_NO_DEVICE
