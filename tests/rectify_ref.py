"""Restatement of the reference's raw-stereo input path in numpy, operation by operation, with explicit
float64 / float32:

  gemm3, invert3         cv::gemm's and cv::invert(DECOMP_LU)'s 3x3 special cases (iR = (Ar*R)^-1)
  init_rectify_map       cv::initUndistortRectifyMap(K, D, R, Ar, size, CV_32FC1)     (ros_stereo.cc:106-107)
  fixed_maps             remap's conversion of float maps for INTER_LINEAR: X = cvRound(m*32), (sat_i16(X >> 5), X & 31)
  remap                  cv::remap(src, M1, M2, INTER_LINEAR, BORDER_CONSTANT 0) on 8U  (ros_stereo.cc:161-162)
  rectify_gray           remap, then GrabImageStereo's cvtColor (src/Tracking.cc:275-310) for 3 / 4 channels
"""
import numpy as np

F32, F64 = np.float32, np.float64
INT_MIN = -2 ** 31

# an EuRoC-like stereo pair (the ORB-SLAM2 examples' EuRoC.yaml): radtan k1 k2 p1 p2, R / P from stereoRectify
EUROC_SIZE = (752, 480)
EUROC_L = dict(K=[[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]],
               D=[-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05],
               R=[[0.999966347530033, -0.001422739138722922, 0.008079580483432283],
                  [0.001365741834644127, 0.9999741760894847, 0.007055629199258132],
                  [-0.008089410156878961, -0.007044357138835809, 0.9999424675829176]],
               P=[[435.2046959714599, 0, 367.4517211914062, 0], [0, 435.2046959714599, 252.2008514404297, 0], [0, 0, 1, 0]])
EUROC_R = dict(K=[[457.587, 0.0, 379.999], [0.0, 456.134, 255.238], [0.0, 0.0, 1]],
               D=[-0.28368365, 0.07451284, -0.00010473, -3.555907e-05],
               R=[[0.9999633526194376, -0.003625811871560086, 0.007755443660172947],
                  [0.003680398547259526, 0.9999684752771629, -0.007035845251224894],
                  [-0.007729688520722713, 0.007064130529506649, 0.999945173484644]],
               P=[[435.2046959714599, 0, 367.4517211914062, -47.90639384423901], [0, 435.2046959714599, 252.2008514404297, 0],
                  [0, 0, 1, 0]])


def gemm3(a, b):
    """cv::gemm 3x3 (alpha 1, no C): d(i,j) = a(i,0)*b(0,j) + a(i,1)*b(1,j) + a(i,2)*b(2,j), left to right, in double."""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    d = np.zeros((3, 3), F64)
    for i in range(3):
        for j in range(3):
            d[i, j] = a[i, 0] * b[0, j] + a[i, 1] * b[1, j] + a[i, 2] * b[2, j]
    return d


def invert3(m):
    """cv::invert(DECOMP_LU) 3x3: det3 by cofactors of row 0, d = 1./d, adjugate * d.  None if d == 0 (singular)."""
    m = np.asarray(m, F64)
    d = (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) +
         m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))
    if d == 0.0:
        return None
    d = F64(1.0) / d
    t = np.zeros(9, F64)
    t[0] = (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) * d
    t[1] = (m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]) * d
    t[2] = (m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]) * d
    t[3] = (m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]) * d
    t[4] = (m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]) * d
    t[5] = (m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]) * d
    t[6] = (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]) * d
    t[7] = (m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]) * d
    t[8] = (m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]) * d
    return t


def dist_coeffs(D):
    """k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 from 4, 5 or 8 coefficients (12 / 14: thin prism / tilt, not supported)."""
    D = [F64(v) for v in np.asarray(D, F64).ravel()]
    if len(D) not in (4, 5, 8):
        raise ValueError("D must have 4, 5 or 8 coefficients, not %d" % len(D))
    z = F64(0.0)
    k3 = D[4] if len(D) >= 5 else z
    k4, k5, k6 = (D[5], D[6], D[7]) if len(D) >= 8 else (z, z, z)
    return D[0], D[1], D[2], D[3], k3, k4, k5, k6, z, z, z, z


def init_rectify_map(K, D, R, P, w, h, f64=False):
    """initUndistortRectifyMap(K, D, R, P[:, :3], (w, h), CV_32FC1) -> (M1, M2) float32 [h, w] (f64: the float64 u, v before the
    cast).  Per row i the recurrence _x = i*ir[1] + ir[2] (_y, _w alike) and, after each pixel, _x += ir[0]: a sequential
    accumulation (np.add.accumulate)."""
    K = np.asarray(K, F64)
    Ar = np.asarray(P, F64)[:, :3]
    ir = invert3(gemm3(Ar, R))
    if ir is None:
        raise ValueError("P[:, :3] * R is singular")
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = dist_coeffs(D)
    u0, v0, fx, fy = K[0, 2], K[1, 2], K[0, 0], K[1, 1]
    i = np.arange(h, dtype=F64)[:, None]

    def run(c0, step):
        seq = np.empty((h, w), F64)
        seq[:, :1] = c0
        seq[:, 1:] = step
        return np.add.accumulate(seq, axis=1)
    _x = run(i * ir[1] + ir[2], ir[0])
    _y = run(i * ir[4] + ir[5], ir[3])
    _w = run(i * ir[7] + ir[8], ir[6])
    with np.errstate(all="ignore"):
        ww = F64(1.0) / _w
        x = _x * ww
        y = _y * ww
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        xd = (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2)
        yd = (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2)
        one, zero = F64(1.0), F64(0.0)
        vt0 = ((zero + one * xd) + zero * yd) + zero * one
        vt1 = ((zero + zero * xd) + one * yd) + zero * one
        vt2 = ((zero + zero * xd) + zero * yd) + one * one
        invProj = np.where(vt2 != 0, one / np.where(vt2 != 0, vt2, one), one)
        u = fx * invProj * vt0 + u0
        v = fy * invProj * vt1 + v0
        return (u, v) if f64 else (u.astype(F32), v.astype(F32))


def cv_round_q5(m):
    """cvRound(m * 32.0f) on x86 (cvtss2si): the float multiply is exact, round half to even; NaN, +-inf and values outside int32
    give INT_MIN."""
    v = np.asarray(m, F32) * F32(32.0)
    ok = np.isfinite(v) & (v >= F32(-2.0 ** 31)) & (v < F32(2.0 ** 31))
    out = np.full(v.shape, INT_MIN, np.int64)
    out[ok] = np.rint(v[ok]).astype(np.int64)
    return out


def fixed_maps(mapx, mapy):
    """remap's fixed-point form: sx = sat_i16(X >> 5), ax = X & 31 (arithmetic shift), likewise sy, ay."""
    X, Y = cv_round_q5(mapx), cv_round_q5(mapy)
    sx = np.clip(X >> 5, -32768, 32767).astype(np.int64)
    sy = np.clip(Y >> 5, -32768, 32767).astype(np.int64)
    return sx, sy, (X & 31).astype(np.int64), (Y & 31).astype(np.int64)


def bilinear_q10(p00, p01, p10, p11, ax, ay):
    """((32-ay)*((32-ax)*p00 + ax*p01) + ay*((32-ax)*p10 + ax*p11) + 512) >> 10"""
    return ((32 - ay) * ((32 - ax) * p00 + ax * p01) + ay * ((32 - ax) * p10 + ax * p11) + 512) >> 10


def bilinear_q15(p, w):
    """OpenCV's form: (sum w_i * p_i + 16384) >> 15 with the 4 Q15 weights of one table entry."""
    return (w[0] * p[0] + w[1] * p[1] + w[2] * p[2] + w[3] * p[3] + (1 << 14)) >> 15


def remap(src, mapx, mapy):
    """remap(src, M1, M2, INTER_LINEAR, BORDER_CONSTANT 0) of an 8-bit [sh, sw] or [sh, sw, c] image: output has the map's size and
    src's channels.  A tap outside the source reads 0; no address is formed from a tap before the range check."""
    src = np.asarray(src, np.uint8)
    squeeze = src.ndim == 2
    s = src[..., None] if squeeze else src
    sh, sw = s.shape[:2]
    sx, sy, ax, ay = fixed_maps(mapx, mapy)

    def tap(x, y):
        inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        v = np.zeros(x.shape + (s.shape[2],), np.int64)
        v[inside] = s[y[inside], x[inside]]
        return v
    p00, p01, p10, p11 = tap(sx, sy), tap(sx + 1, sy), tap(sx, sy + 1), tap(sx + 1, sy + 1)
    out = bilinear_q10(p00, p01, p10, p11, ax[..., None], ay[..., None]).astype(np.uint8)
    return out[..., 0] if squeeze else out


def gray_from_color(img, rgb=True):
    """OpenCV's 8-bit RGB2Gray (item 5): Y = (R*4899 + G*9617 + B*1868 + 8192) >> 14."""
    c = img.astype(np.int32)
    r, g, b = (c[..., 0], c[..., 1], c[..., 2]) if rgb else (c[..., 2], c[..., 1], c[..., 0])
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def rectify_gray(src, mapx, mapy, rgb=True):
    """The reference's order: remap every channel, then cvtColor to gray (1 channel: the remapped image)."""
    out = remap(src, mapx, mapy)
    return out if out.ndim == 2 else gray_from_color(out, rgb)
