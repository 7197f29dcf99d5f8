"""CPU: the numpy restatement of the dense keyframe cloud (tests/cloud_ref.py) against hand-derived answers, and the cloud part of
the C ABI where no GPU is needed (argument errors, sizes, the loud failure without a device)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ref as R   # noqa: E402

F32 = np.float32
I4 = np.eye(4)


cloud, order_sensitive_cloud = R.make_cloud, R.order_sensitive_cloud


# ---- generate

def test_depth_gate_boundaries():
    assert float(F32(0.01)) < 0.01 and not R.depth_gate(F32(0.01))           # 0.01f = 0.00999999977...: below the double literal
    assert R.depth_gate(np.nextafter(F32(0.01), F32(1)))
    assert R.depth_gate(F32(10.0))
    assert not R.depth_gate(np.nextafter(F32(10.0), F32(np.inf)))
    assert R.depth_gate(F32(np.nan))                                   # both comparisons are false: kept
    for v in (np.inf, -np.inf, 0.0, -0.0, -1.0, 1e-3):
        assert not R.depth_gate(F32(v)), v


def test_generate_gate_and_nan_point():
    d = np.array([[0.01, 10.0, np.nextafter(F32(10.0), F32(np.inf)), np.nan, np.inf, -np.inf, 0.0, -2.0, 1.0]], F32)
    c = np.zeros((1, 9, 3), np.uint8)
    c[0, :, 0] = np.arange(9)
    p = R.generate(c, d, 2.0, 2.0, 0.0, 0.0, I4, step=1)
    assert list(p["b"]) == [1, 3, 8]                                   # 10.0f, NaN and 1.0 survive, in scan order
    assert p["z"][0] == F32(10.0) and p["x"][0] == F32(5.0)            # (1 - 0) * 10 / 2
    assert np.isnan(p["x"][1]) and np.isnan(p["y"][1]) and np.isnan(p["z"][1])
    assert p["x"][2] == F32(4.0) and p["y"][2] == F32(0.0) and (p["a"] == 255).all()


@pytest.mark.parametrize("step", [1, 2, 3])
def test_scan_order_and_step_on_a_size_that_is_no_multiple(step):
    w, h = 7, 5
    depth = np.ones((h, w), F32)
    color = np.zeros((h, w, 3), np.uint8)
    color[..., 0] = np.arange(w)[None, :]
    color[..., 1] = np.arange(h)[:, None]
    color[..., 2] = 77
    p = R.generate(color, depth, 1.0, 1.0, 0.0, 0.0, I4, step=step, alpha=9)
    ms, ns = list(range(0, h, step)), list(range(0, w, step))
    assert len(p) == len(ms) * len(ns) == R.capacity(w, h, step)
    assert list(p["g"]) == [m for m in ms for n in ns] and list(p["b"]) == [n for m in ms for n in ns]   # rows outside, columns inside
    assert (p["r"] == 77).all() and (p["a"] == 9).all()
    assert list(p["x"]) == [float(n) for m in ms for n in ns] and list(p["y"]) == [float(m) for m in ms for n in ns]


def test_identity_pose_and_dyadic_pose():
    depth = np.array([[2.0, 4.0], [0.5, 8.0]], F32)
    color = np.zeros((2, 2, 3), np.uint8)
    a = R.generate(color, depth, 4.0, 2.0, 0.5, 0.25, I4, step=1)
    # x = (n - 0.5) * z / 4, y = (m - 0.25) * z / 2
    assert list(a["x"]) == [-0.25, 0.5, -0.0625, 1.0] and list(a["y"]) == [-0.25, -0.5, 0.1875, 3.0]
    assert list(a["z"]) == [2.0, 4.0, 0.5, 8.0]
    M = np.array([[0, -1, 0, 0.5], [0.5, 0, 0, -2], [0, 0, 2, 0.25], [0, 0, 0, 1]], np.float64)
    b = R.generate(color, depth, 4.0, 2.0, 0.5, 0.25, M, step=1)
    assert list(b["x"]) == [0.75, 1.0, 0.3125, -2.5]                  # -y + 0.5
    assert list(b["y"]) == [-2.125, -1.75, -2.03125, -1.5]           # x / 2 - 2
    assert list(b["z"]) == [4.25, 8.25, 1.25, 16.25]                 # 2 z + 0.25


def test_u16_depth_uses_the_rgbd_conversion_rule():
    depth = np.array([[5000, 0, 50000, 50001]], np.uint16)
    p = R.generate(np.zeros((1, 4, 3), np.uint8), depth, 1.0, 1.0, 0.0, 0.0, I4, factor=1.0 / 5000.0, step=1)
    f = F32(1.0 / 5000.0)
    kept = [v for v in (5000, 50000, 50001) if R.depth_gate(F32(F32(v) * f))]
    assert list(p["z"]) == [F32(F32(v) * f) for v in kept] and 5000 in kept
    # an F32 image with factor 1 is taken as it is; with another factor it is multiplied
    d32 = np.array([[1.5]], F32)
    assert R.generate(np.zeros((1, 1, 3), np.uint8), d32, 1.0, 1.0, 0.0, 0.0, I4, factor=1.0, step=1)["z"][0] == F32(1.5)
    assert R.generate(np.zeros((1, 1, 3), np.uint8), d32, 1.0, 1.0, 0.0, 0.0, I4, factor=2.0, step=1)["z"][0] == F32(3.0)


# ---- voxel

def test_voxel_floor_at_negative_coordinates():
    # leaf 1: -0.5 lies in cell -1, 0.5 in cell 0: two voxels, not one (truncation would merge them)
    out, n = R.voxel(cloud([[0.5, 0, 0], [-0.5, 0, 0]]), 1.0)
    assert n == 2 and list(out["x"]) == [-0.5, 0.5]                  # ascending cell index, not input order
    out, n = R.voxel(cloud([[-0.25, -0.25, -0.25], [-0.75, -0.75, -0.75]]), 1.0)
    assert n == 1 and out["x"][0] == F32(-0.5)


def test_voxel_point_on_a_cell_face():
    # x = 1.0 exactly at leaf 0.5 (inv = 2 exactly): floor(2.0) = 2, the cell above the face; 0.999 stays in cell 1
    out, n = R.voxel(cloud([[1.0, 0, 0], [0.999, 0, 0], [0.5, 0, 0]]), 0.5)
    assert n == 2 and list(out["x"]) == [F32((F32(0.999) + F32(0.5)) / F32(2)), F32(1.0)]


def test_voxel_colour_mean_truncates():
    out, n = R.voxel(cloud([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2]], [[255, 1, 0, 255], [254, 2, 0, 254]]), 1.0)
    assert n == 1 and (out["r"][0], out["g"][0], out["b"][0], out["a"][0]) == (254, 1, 0, 254)   # 254.5 -> 254, 1.5 -> 1


def test_voxel_drops_nan_and_inf_points():
    pts = cloud([[0.1, 0.1, 0.1], [np.nan, 0, 0], [0, np.inf, 0], [0.3, 0.3, 0.3], [0, 0, -np.inf]], [[10, 0, 0, 0]] * 5)
    out, n = R.voxel(pts, 1.0)
    assert n == 1 and out["x"][0] == F32((F32(0.1) + F32(0.3)) / F32(2))
    assert R.voxel(cloud([[np.nan, 0, 0]]), 1.0)[1] == 0 and R.voxel(cloud(np.zeros((0, 3))), 1.0)[1] == 0


def test_voxel_overflow_case():
    # 10 m along every axis at leaf 1e-4: 100001^3 cells > INT32_MAX
    out, n = R.voxel(cloud([[0, 0, 0], [10, 10, 10]]), 1e-4)
    assert n == -1 and len(out) == 0
    assert R.voxel(cloud([[0, 0, 0], [10, 10, 10]]), 1e-2)[1] == 2   # 1001^3 fits


def test_voxel_sum_is_sequential_and_the_case_discriminates():
    pts, x = order_sensitive_cloud()
    seq, tree = R.seq_sum_f32(x), R.pairwise_sum_f32(x)
    assert seq == F32(10000.0625) and tree != seq and abs(float(tree) - 10000.064) < 1e-3
    out, n = R.voxel(pts, 1e5)
    assert n == 1 and out["x"][0] == F32(seq / F32(65)) and out["x"][0] != F32(tree / F32(65))


def test_voxel_output_is_in_ascending_cell_index_with_y_and_z_strides():
    # 2 x 2 x 2 cells of leaf 1: idx = i + 2 j + 4 k
    pts = cloud([[1.5, 1.5, 1.5], [0.5, 1.5, 0.5], [1.5, 0.5, 0.5], [0.5, 0.5, 1.5], [0.5, 0.5, 0.5]])
    out, n = R.voxel(pts, 1.0)
    assert n == 5 and [tuple(map(float, (p["x"], p["y"], p["z"]))) for p in out] == [
        (0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, 1.5, 0.5), (0.5, 0.5, 1.5), (1.5, 1.5, 1.5)]


# ---- C ABI without a GPU

def test_cloud_abi_sizes(pkg):
    assert hasattr(pkg, "CloudMapper")
    assert pkg.CLOUD_DTYPE.itemsize == 16 and pkg.CLOUD_DTYPE == R.CLOUD_DTYPE
    assert pkg.cloud_capacity(61, 47, 3) == 21 * 16 == R.capacity(61, 47, 3)
    assert pkg.cloud_capacity(640, 480, 3) == 214 * 160 and pkg.cloud_capacity(640, 480, 1) == 640 * 480


def test_cloud_argument_errors_come_before_the_device(pkg):
    L = pkg.lib()
    m = C.c_void_p()
    for leaf, step, alpha in ((0.0, 3, 255), (-0.1, 3, 255), (0.1, 0, 255), (0.1, 3, -1), (0.1, 3, 256)):
        assert L.orbx_cloudmapper_create(leaf, step, alpha, 0, C.byref(m)) == pkg.ORBX_ERR_ARG, (leaf, step, alpha)
    assert L.orbx_cloudmapper_create(0.1, 3, 255, 0, None) == pkg.ORBX_ERR_ARG
    assert L.orbx_cloudmapper_destroy(None) == 0
    with pytest.raises(pkg.OrbxError) as e:
        pkg.CloudMapper(leaf=0.0)
    assert e.value.status == pkg.ORBX_ERR_ARG
    assert L.orbx_cloud_voxel_device(None, None, None, 1, 1, None, 1, None, None) == pkg.ORBX_ERR_ARG
    assert L.orbx_keyframe_cloud(None, None, 3, 0, None, 5, 0, 1.0, 0, 0, 1.0, 1.0, 0.0, 0.0, None, 0, None, None, None, None) == pkg.ORBX_ERR_ARG


def test_cloud_mapper_without_a_gpu_fails_loudly(pkg):
    if pkg.device_count() > 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(pkg.OrbxError) as e:
        pkg.CloudMapper(0.1, 3, 255)
    assert e.value.status == pkg.ORBX_ERR_NO_DEVICE
