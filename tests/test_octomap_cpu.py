"""CPU: the restatement of the reference's occupancy octree (tests/octomap_ref.py) against known answers worked out by hand from
octomap's file format, its two forms against each other, and the host-side part of the C ABI (no device needed)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import octomap_ref as R   # noqa: E402

F32 = np.float32
H = bytes.fromhex


def grid(vals):
    return np.array([[x, y, z] for z in vals for y in vals for x in vals], F32)


B2, B4 = grid([0.05, 0.15]), grid([0.05, 0.15, 0.25, 0.35])
# (points, data bytes or None, size, length of the data, its head, its tail): M = identity, res = 0.1
KNOWN = {
    "one_point_pos": ([[0.05, 0.05, 0.05]], H("00c0") + 14 * H("0300") + H("0200"), 17),
    "one_point_neg": ([[-0.05, -0.05, -0.05]], H("0300") + 14 * H("00c0") + H("0080"), 17),
    "block_2": (B2, H("00c0") + 13 * H("0300") + H("0200"), 16),
    "block_2_shifted_x": (B2 + F32([0.1, 0, 0]), H("00c0") + 13 * H("0300") + H("0f00") + H("8888") + H("2222"), 25),
    "block_4": (B4, H("00c0") + 12 * H("0300") + H("0200"), 15),
    "block_4_minus_last": (B4[:-1], None, 30),
    "eight_octants": (grid([-0.05, 0.05]), None, 129),
}
# float32 x at y = z = 0 -> its key, or None where the point is dropped
BOUNDARY = [(3276.7998, 65535), (3276.8, None), (-3276.8, None), (-3276.8003, None), (np.inf, None), (-np.inf, None), (np.nan, None),
            (0.3, 32771), (-0.0, 32768), (0.0, 32768), (-3276.7998, 0), (-1e-30, 32767)]


@pytest.mark.parametrize("name", sorted(KNOWN))
def test_known_answers(name):
    pts, data, size = KNOWN[name]
    for form in (R.octomap, R.levelwise):
        r = form(pts, R.IDENTITY, 0.1)
        assert r["tree_size"] == size and r["points_dropped"] == 0 and r["data_bytes"] == len(r["data"])
        if data is not None:
            assert r["data"] == data
        assert r["tree_size"] == r["data_bytes"] // 2 + r["leaves"]
    r = R.octomap(pts, R.IDENTITY, 0.1)
    if name == "block_4_minus_last":
        assert len(r["data"]) == 32 and r["data"].endswith(H("0300aaeaaa2a")) and r["leaves"] == 14
    if name == "eight_octants":
        assert len(r["data"]) == 242 and r["data"].startswith(H("ffff")) and r["leaves"] == 8
    if name == "block_2":
        assert r["leaf_rows"].tolist() == [[32768, 32768, 32768, 15]]
    if name == "block_4":
        assert r["leaf_rows"].tolist() == [[32768, 32768, 32768, 14]] and r["cells"] == 64


def test_key_boundaries():
    for x, key in BOUNDARY:
        k, dropped = R.point_keys(np.array([[x, 0, 0]], F32), R.IDENTITY, 0.1)
        if key is None:
            assert dropped == 1 and len(k) == 0, x
        else:
            assert dropped == 0 and k.tolist() == [[key, 32768, 32768]], x
    assert 10.0 * float(F32(0.3)) > 3.0 and 1.0 / 0.1 == 10.0
    # a non-finite y or z drops the point as well, and the file of a map with nothing left is the header alone
    r = R.octomap(np.array([[0, np.nan, 0], [0, 0, np.inf], [4000, 0, 0]], F32), R.IDENTITY, 0.1)
    assert r["points_dropped"] == 3 and r["tree_size"] == 0 and r["data"] == b"" and r["file"] == R.header(0, 0.1)


def test_header_text():
    assert R.header(17, 0.1) == (b"# Octomap OcTree binary file\n# (feel free to add / change comments, but leave the first line as it is!)\n"
                                 b"#\nid OcTree\nsize 17\nres 0.1\ndata\n")
    assert R.header(0, 0.05) == (b"# Octomap OcTree binary file\n# (feel free to add / change comments, but leave the first line as it is!)\n"
                                 b"#\nid OcTree\nsize 0\nres 0.05\ndata\n")
    assert R.octomap([[0.05, 0.05, 0.05]], R.IDENTITY, 0.05)["file"].startswith(R.header(17, 0.05))


def random_points(n, seed=3, side=5.0):
    rng = np.random.default_rng(seed)
    p = (rng.random((n, 3)) * 2 * side - side).astype(F32)
    p[n - n // 3:] = p[:n // 3]   # a third are duplicates of others
    return p


def test_round_trip_and_the_two_forms_agree():
    pts = np.concatenate([random_points(5000), B4 + F32([1.6, -3.2, 0.8]), grid(np.arange(-4, 5) * 0.1 + 0.05)])
    for M, res in ((R.AXIS_SWAP, 0.1), (R.IDENTITY, 0.25)):
        a, b = R.octomap(pts, M, res), R.levelwise(pts, M, res)
        for f in ("points_in", "points_dropped", "cells", "leaves", "tree_size", "data_bytes", "data", "file"):
            assert a[f] == b[f], f
        assert (a["leaf_rows"] == b["leaf_rows"]).all()
        size, r, leaves = R.read_bt(a["file"])
        assert size == a["tree_size"] and r == res
        assert leaves == {tuple(l) for l in a["leaf_rows"].tolist()} and len(leaves) == a["leaves"]
        if res == 0.1:
            assert {int(d) for d in a["leaf_rows"][:, 3]} >= {14, 16}   # the 4 x 4 x 4 blocks of the origin grid, and single cells
    assert R.read_bt(R.header(0, 0.1)) == (0, 0.1, set())


def test_default_matrix_is_the_product_of_the_three(pkg):
    M = R.TRANS @ R.ROT_X @ R.ROT_Y
    assert (M == R.AXIS_SWAP).all() and (pkg.OCTOMAP_AXIS_SWAP == R.AXIS_SWAP).all() and pkg.OCTOMAP_AXIS_SWAP.dtype == F32
    p, fin = R.transform([[1, 2, 3]], R.AXIS_SWAP)
    assert p.tolist() == [[3, -1, -2]] and fin.all()
    assert pkg.OCTREE_LEAF_DTYPE.itemsize == 8 and C.sizeof(pkg.OctreeInfo) == 56


def test_abi_without_a_device(pkg):
    L = pkg.lib()
    assert L.orbx_octomap_bytes_bound(-1) == 0 and L.orbx_octomap_bytes_bound(0) == 192
    for n in (1, 7, 1 << 27):
        assert L.orbx_octomap_bytes_bound(n) == 192 + 2 * (15 * n + 1)
    assert len(R.header(2 ** 31, 1.0 / 3)) <= 192
    fake = C.create_string_buffer(4096)   # stands in for a mapper: the argument checks come before anything looks at it
    m = C.cast(fake, C.c_void_p)
    pts, out, nb, info = np.zeros(4, pkg.CLOUD_DTYPE), np.zeros(512, np.uint8), C.c_size_t(), pkg.OctreeInfo()
    p, o = pts.ctypes.data, out.ctypes.data
    for res in (0.0, -0.1, float("nan"), float("inf")):
        assert L.orbx_octomap_bt(m, p, 4, None, res, o, 512, C.byref(nb), C.byref(info)) == pkg.ORBX_ERR_ARG
        assert L.orbx_octree_device(m, p, p, 1, 4, None, res, o, 512, None, 0, o, None) == pkg.ORBX_ERR_ARG
    assert b"orbx_octree_device" in L.orbx_last_error()
    assert L.orbx_octomap_bt(m, p, -1, None, 0.1, o, 512, C.byref(nb), C.byref(info)) == pkg.ORBX_ERR_ARG
    assert L.orbx_octomap_bt(m, None, 4, None, 0.1, o, 512, C.byref(nb), C.byref(info)) == pkg.ORBX_ERR_ARG
    assert L.orbx_octomap_bt(m, p, 4, None, 0.1, None, 512, C.byref(nb), C.byref(info)) == pkg.ORBX_ERR_ARG
    assert L.orbx_octomap_bt(m, p, 4, None, 0.1, o, 512, None, C.byref(info)) == pkg.ORBX_ERR_ARG
    assert L.orbx_octomap_bt(None, p, 4, None, 0.1, o, 512, C.byref(nb), C.byref(info)) == pkg.ORBX_ERR_ARG
    assert b"orbx_octomap_bt" in L.orbx_last_error()
    assert L.orbx_octree_device(m, p, p, 0, 4, None, 0.1, o, 512, None, 0, o, None) == pkg.ORBX_ERR_ARG
    assert L.orbx_octree_device(m, p, p, 1, 4, None, 0.1, o, 512, None, 0, None, None) == pkg.ORBX_ERR_ARG
    assert L.orbx_octree_device(m, p, p, 1, 4, None, 0.1, o, -1, None, 0, o, None) == pkg.ORBX_ERR_ARG
    assert L.orbx_octree_device(m, p, p, 1 << 14, 1 << 14, None, 0.1, o, 512, None, 0, o, None) == pkg.ORBX_ERR_ARG   # B * cap > 2^27
    # an empty map needs no device: the header with size 0
    for res in (0.1, 0.05):
        assert L.orbx_octomap_bt(m, None, 0, None, res, o, 512, C.byref(nb), C.byref(info)) == pkg.ORBX_OK
        assert out[:nb.value].tobytes() == R.header(0, res) and info.as_dict() == dict(
            points_in=0, points_dropped=0, cells=0, leaves=0, tree_size=0, data_bytes=0, overflow=0)
    assert L.orbx_octomap_bt(m, None, 0, None, 0.1, o, 10, C.byref(nb), None) == pkg.ORBX_ERR_CAPACITY and nb.value == len(R.header(0, 0.1))
