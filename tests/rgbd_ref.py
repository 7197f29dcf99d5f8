"""Restatement of the reference's RGB-D front end in numpy, operation by operation, with explicit float32 / float64:

  gray_from_color      Tracking::GrabImageRGBD's cvtColor (src/Tracking.cc:315-333): OpenCV's 8-bit RGB2Gray
  depth_converts       the convertTo rule of GrabImageRGBD (:335-336)
  undistort_points     Frame::UndistortKeyPoints (src/Frame.cc:419-449) = cv::undistortPoints(pts, K, D, noArray(), K), OpenCV 3.2
  rgbd_assoc           UndistortKeyPoints + ComputeStereoFromRGBD (src/Frame.cc:658-679)
  compute_image_bounds Frame::ComputeImageBounds (src/Frame.cc:451-479)
  distort_points       the forward distortion model (cv::projectPoints' arithmetic) - for round-trip checks only
"""
import numpy as np

F32, F64 = np.float32, np.float64
DEPTH_U16, DEPTH_F32 = 2, 5

# TUM RGB-D fr1 calibration (the ORB-SLAM2 examples' TUM1.yaml)
TUM1 = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, k1=0.262383, k2=-0.953104, p1=-0.005358, p2=0.002628,
            k3=1.163314, mbf=40.0)
# the reference's own settings (config/Asus.yaml): no distortion
ASUS = dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, mbf=40.0)


def gray_from_color(img, rgb=True):
    """uint8 [h, w, 3|4] -> uint8 [h, w]: Y = (R*4899 + G*9617 + B*1868 + 8192) >> 14, R/B by channel order."""
    c = img.astype(np.int32)
    r, g, b = (c[..., 0], c[..., 1], c[..., 2]) if rgb else (c[..., 2], c[..., 1], c[..., 0])
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def depth_converts(depth_dtype, factor):
    """if (fabs(mDepthMapFactor-1.0f) > 1e-5 || mImDepth.type() != CV_32F) convertTo(CV_32F, mDepthMapFactor)"""
    f = F32(factor)
    return bool(F64(abs(f - F32(1.0))) > 1e-5) or np.dtype(depth_dtype) != np.float32


def depth_sample(depth, u, v, factor):
    """imDepth.at<float>(v, u) after GrabImageRGBD's conversion: (float)raw * factor, one rounded float multiply."""
    raw = depth[v, u]
    if depth_converts(depth.dtype, factor):
        return F32(F32(raw) * F32(factor))
    return F32(raw)


def _cam64(cam):
    return {k: F64(F32(v)) for k, v in cam.items()}


def undistort_points(x, y, cam):
    """cvUndistortPoints (OpenCV 3.2) with R = I, P = K: five iterations in double, every term of the 3.2 expression written out,
    the exactly-zero ones included (tilt = I, k4..k6 = 0, s1..s4 = 0, RR = K); float32 in and out.  Not modelled: the icdist < 0
    early exit of later releases (only reachable far outside real lens distortion)."""
    c = _cam64(cam)
    k = [c["k1"], c["k2"], c["p1"], c["p2"], c["k3"], F64(0), F64(0), F64(0), F64(0), F64(0), F64(0), F64(0)]
    fx, fy, cx, cy = c["fx"], c["fy"], c["cx"], c["cy"]
    ifx, ify = F64(1.0) / fx, F64(1.0) / fy
    x = np.asarray(x, F32).astype(F64)
    y = np.asarray(y, F32).astype(F64)
    x = (x - cx) * ifx
    y = (y - cy) * ify
    one, zero = F64(1.0), F64(0.0)
    ux = one * x + zero * y + zero * one
    uy = zero * x + one * y + zero * one
    uz = zero * x + zero * y + one * one
    inv_proj = np.where(uz != 0, one / uz, one)
    x0 = inv_proj * ux
    y0 = inv_proj * uy
    x, y = x0, y0
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        delta_x = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
        delta_y = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x = (x0 - delta_x) * icdist
        y = (y0 - delta_y) * icdist
    xx = fx * x + zero * y + cx
    yy = zero * x + fy * y + cy
    ww = one / (zero * x + zero * y + one)
    return (xx * ww).astype(F32), (yy * ww).astype(F32)


def distort_points(x, y, cam):
    """Forward model: undistorted pixel -> distorted pixel (k1 k2 p1 p2 k3), in float64."""
    c = {k: float(F32(v)) for k, v in cam.items()}
    xn = (np.asarray(x, F64) - c["cx"]) / c["fx"]
    yn = (np.asarray(y, F64) - c["cy"]) / c["fy"]
    r2 = xn * xn + yn * yn
    radial = 1 + c["k1"] * r2 + c["k2"] * r2 * r2 + c["k3"] * r2 * r2 * r2
    xd = xn * radial + 2 * c["p1"] * xn * yn + c["p2"] * (r2 + 2 * xn * xn)
    yd = yn * radial + c["p1"] * (r2 + 2 * yn * yn) + 2 * c["p2"] * xn * yn
    return xd * c["fx"] + c["cx"], yd * c["fy"] + c["cy"]


def undistort_keypoints(kp, cam):
    """Frame::UndistortKeyPoints: a no-op iff mDistCoef.at<float>(0) == 0.0 (k1 only, whatever p1 / p2 are)."""
    kun = kp.copy()
    if F32(cam["k1"]) == F32(0.0) or len(kp) == 0:
        return kun
    kun["x"], kun["y"] = undistort_points(kp["x"], kp["y"], cam)
    return kun


def rgbd_assoc(kp, depth, factor, cam):
    """-> (kun, uright, depth): mvKeysUn, then ComputeStereoFromRGBD at the DISTORTED keypoint (u, v truncated to int);
    depth None = the monocular constructor's tail (-1 / -1)."""
    kun = undistort_keypoints(kp, cam)
    n = len(kp)
    ur, dp = np.full(n, -1, F32), np.full(n, -1, F32)
    if depth is None:
        return kun, ur, dp
    mbf = F32(cam["mbf"])
    h, w = depth.shape
    for i in range(n):
        u, v = int(kp["x"][i]), int(kp["y"][i])
        if not (0 <= u < w and 0 <= v < h):
            continue
        d = depth_sample(depth, u, v, factor)
        if d > 0:
            dp[i] = d
            ur[i] = F32(kun["x"][i] - F32(mbf / d))
    return kun, ur, dp


def compute_image_bounds(w, h, cam):
    """Frame::ComputeImageBounds -> (mnMinX, mnMaxX, mnMinY, mnMaxY) as float32."""
    if F32(cam["k1"]) != F32(0.0):
        x, y = undistort_points(np.array([0, w, 0, w], F32), np.array([0, 0, h, h], F32), cam)
        return min(x[0], x[2]), max(x[1], x[3]), min(y[0], y[1]), max(y[2], y[3])
    return F32(0), F32(w), F32(0), F32(h)
