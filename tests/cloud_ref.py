"""Restatement of the reference's dense RGB-D keyframe cloud in numpy, operation by operation, with explicit
float32 / float64:

  generate   PointCloudMapping::generatePointCloud (src/pointcloudmapping.cc:83-114): the sampled grid, the depth gate, the
             back-projection, pcl::transformPointCloud with a double 4x4
  voxel      pcl::VoxelGrid<pcl::PointXYZRGBA>::applyFilter as of PCL 1.8 (downsample_all_data, no filter field,
             min_points_per_voxel 0, input not dense) as saveOctomap runs it (:117-127)

The choices a real PCL / Eigen / libstdc++ build could make differently (tie order of std::sort, vector / scalar as a division,
floor - min_b in float, the default alpha, no FMA contraction) are listed in DESIGN.md §3.
"""
import numpy as np

import rgbd_ref

F32, F64 = np.float32, np.float64
CLOUD_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("b", "u1"), ("g", "u1"), ("r", "u1"), ("a", "u1")])
INT32_MAX = 2147483647


def capacity(w, h, step=3):
    return -(-w // step) * -(-h // step)


def depth_gate(d):
    """False = `if (d < 0.01 || d > 10) continue;`: the float is promoted to double and compared with double literals.  NaN passes."""
    d = F64(F32(d))
    return not (d < F64(0.01) or d > F64(10.0))


def depth_plane(depth, factor):
    """mImDepth after GrabImageRGBD's conversion (rgbd_ref.depth_sample for every pixel)."""
    if rgbd_ref.depth_converts(depth.dtype, factor):
        return (depth.astype(F32) * F32(factor)).astype(F32)
    return depth.astype(F32)


def generate(color, depth, fx, fy, cx, cy, Twc, factor=1.0, step=3, alpha=255):
    """color uint8 [h, w, 3|4], depth uint16 / float32 [h, w], Twc 4x4 double -> CLOUD_DTYPE array in scan order."""
    h, w = depth.shape
    fx, fy, cx, cy = F32(fx), F32(fy), F32(cx), F32(cy)
    M = np.asarray(Twc, F64).reshape(4, 4)
    dp = depth_plane(depth, factor)
    mm, nn = np.meshgrid(np.arange(0, h, step), np.arange(0, w, step), indexing="ij")
    mm, nn = mm.ravel(), nn.ravel()
    with np.errstate(all="ignore"):
        d = dp[mm, nn]
        d64 = d.astype(F64)
        keep = ~((d64 < F64(0.01)) | (d64 > F64(10.0)))
        mm, nn, z = mm[keep], nn[keep], d[keep]
        x = ((nn.astype(F32) - cx) * z / fx).astype(F32)
        y = ((mm.astype(F32) - cy) * z / fy).astype(F32)
        xd, yd, zd = x.astype(F64), y.astype(F64), z.astype(F64)
        out = np.zeros(len(z), CLOUD_DTYPE)
        for k, f in enumerate("xyz"):
            out[f] = (((M[k, 0] * xd + M[k, 1] * yd) + M[k, 2] * zd) + M[k, 3]).astype(F32)
    out["b"], out["g"], out["r"] = color[mm, nn, 0], color[mm, nn, 1], color[mm, nn, 2]
    out["a"] = alpha
    return out


def seq_sum_f32(v):
    """((v0 + v1) + v2) + ... in float32, starting from 0.0f."""
    s = F32(0.0)
    for e in np.asarray(v, F32):
        s = F32(s + e)
    return s


def pairwise_sum_f32(v):
    """A balanced tree of float32 additions: what a parallel reduction would give."""
    v = list(np.asarray(v, F32))
    while len(v) > 1:
        v = [F32(v[i] + v[i + 1]) if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
    return v[0] if v else F32(0.0)


def voxel_indices(pts, leaf):
    """-> (finite input indices, idx per finite point as uint32, 0) or (None, None, -1) on the overflow case."""
    inv = F32(1.0) / F32(leaf)
    xyz = np.stack([pts["x"], pts["y"], pts["z"]], 1).astype(F32)
    fin = np.flatnonzero(np.isfinite(xyz).all(1))
    if len(fin) == 0:
        return fin, np.zeros(0, np.uint32), 0
    p = xyz[fin]
    mn, mx = p.min(0), p.max(0)
    with np.errstate(all="ignore"):
        ext = ((mx - mn).astype(F32) * inv).astype(F32)
    d = []
    for e in ext:
        if not e < F32(2147483648.0):   # the cast itself would overflow: more cells along one axis than the product may have
            return None, None, -1
        d.append(int(e) + 1)
    if d[0] * d[1] * d[2] > INT32_MAX:
        return None, None, -1
    min_b = np.floor((mn * inv).astype(F32)).astype(np.int64)
    max_b = np.floor((mx * inv).astype(F32)).astype(np.int64)
    div_b = max_b - min_b + 1
    mul = np.array([1, div_b[0], div_b[0] * div_b[1]], np.int64)
    ijk = (np.floor((p * inv).astype(F32)).astype(F32) - min_b.astype(F32)).astype(F32).astype(np.int64)
    idx = ((ijk * mul).sum(1) & 0xFFFFFFFF).astype(np.uint32)   # (stored as unsigned int)
    return fin, idx, 0


def voxel(pts, leaf):
    """-> (CLOUD_DTYPE array, count); count -1 = the grid overflows (PCL warns and returns its input), array empty."""
    fin, idx, st = voxel_indices(pts, leaf)
    if st < 0:
        return np.zeros(0, CLOUD_DTYPE), -1
    order = np.argsort(idx, kind="stable")
    sidx = idx[order]
    heads = np.flatnonzero(np.r_[True, sidx[1:] != sidx[:-1]]) if len(sidx) else np.zeros(0, np.int64)
    ends = np.r_[heads[1:], len(sidx)]
    out = np.zeros(len(heads), CLOUD_DTYPE)
    if len(heads) == 0:
        return out, 0
    rows = pts[fin[order]]
    fields = ("x", "y", "z", "r", "g", "b", "a")
    vals = np.stack([rows[f].astype(F32) for f in fields], 1)
    lens = ends - heads
    sums = np.zeros((len(heads), 7), F32)
    with np.errstate(all="ignore"):
        for j in range(int(lens.max())):   # the j-th point of every voxel that has one: sequential float32 sums, voxels side by side
            sel = np.flatnonzero(lens > j)
            sums[sel] = (sums[sel] + vals[heads[sel] + j]).astype(F32)
        mean = (sums / lens.astype(F32)[:, None]).astype(F32)
    for k, f in enumerate(fields):
        out[f] = mean[:, k] if k < 3 else mean[:, k].astype(np.uint32).astype(np.uint8)   # (uint8)(uint32): truncation
    return out, len(out)


def same_points(a, b):
    """Bit for bit, except that a NaN matches any NaN (payloads differ between hosts)."""
    if len(a) != len(b):
        return False
    for f in "xyz":
        x, y = a[f], b[f]
        nan = np.isnan(x)
        if not (nan == np.isnan(y)).all() or x[~nan].tobytes() != y[~nan].tobytes():
            return False
    return all((a[f] == b[f]).all() for f in "bgra")


def make_cloud(xyz, rgba=None):
    """[n, 3] coordinates (+ [n, 4] r g b a) -> CLOUD_DTYPE array."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    p = np.zeros(len(xyz), CLOUD_DTYPE)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if rgba is not None:
        rgba = np.asarray(rgba, np.uint8).reshape(-1, 4)
        p["r"], p["g"], p["b"], p["a"] = rgba[:, 0], rgba[:, 1], rgba[:, 2], rgba[:, 3]
    return p


def order_sensitive_cloud():
    """One voxel (leaf 1e5 around the origin) whose float sum depends on the order: 1e4 is followed by 64 times 1e-3; the ulp of
    1e4 is 2^-10 = 0.00097656, so each 1e-3 added alone is rounded to one ulp (the sum ends at 1e4 + 64 * 2^-10 = 10000.0625), while a
    tree adds the small terms up first (0.064) and rounds once.  -> (cloud, its x column)"""
    x = np.r_[F32(1e4), np.full(64, 1e-3, F32)]
    return make_cloud(np.stack([x, np.zeros(65, F32), np.zeros(65, F32)], 1)), x
