"""GPU: dense keyframe clouds (orb_slam2v2-1_amd/csrc/orbx_cloud.hip) against the numpy restatement tests/cloud_ref.py, bit for bit:
points, their order and the counts.  Where the restatement gives NaN the GPU must give NaN; nothing else has a tolerance."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cloud_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
CAM = dict(fx=535.4, fy=539.2, cx=320.1, cy=247.6)   # config/Asus.yaml
SENT = 0x5A


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def pose(k):
    """A rigid 4x4 in double (what toSE3Quat(GetPose()).inverse().matrix() hands over); k = 0: entries with long mantissas."""
    a, b, c = 0.3 + 0.41 * k, -0.2 + 0.17 * k, 0.11 - 0.23 * k
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = rx @ ry @ rz
    M[:3, 3] = [0.7 - k, 1.3 * k - 0.4, 0.05 + 0.6 * k]
    return M


def colour_image(w, h, channels, k=0):
    y, x = np.mgrid[0:h, 0:w]
    ch = [(x * 3 + y + k) & 255, (x + y * 5 + 2 * k) & 255, (x * y + k) & 255] + ([(x + 77) & 255] if channels == 4 else [])
    return np.stack(ch, -1).astype(np.uint8)


def depth_image(w, h, kind, k=0, mode="holes"):
    """mode holes: a scene with holes of every kind, regular ones and a block of rows long enough that whole wavefronts of samples
    are empty at every step; none: no sample passes the gate; all: every sample does."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    metres = 1.0 + 1.5 * x / w + 0.7 * y / h + 0.05 * np.sin(x * 0.37 + y * 0.11 + k)
    xi, yi = x.astype(int), y.astype(int)
    hole = ((xi * 7 + yi * 13) % 5) == 0
    run = (yi >= h // 5) & (yi < h // 5 + max(h // 2, 1))   # (61 x 47 at step 3: 8 sampled rows of 21 = 168 samples in a row)
    if kind == "u16":
        d = np.round(metres * 5000).astype(np.uint16)
        if mode == "none":
            d[:] = 0
            d[::2, ::3] = 60000          # 12 m
        elif mode == "holes":
            d[hole] = np.where((xi + yi) % 2 == 0, 0, 50001 + (xi % 9000))[hole]   # 0 and beyond 10 m
            d[run] = np.where(xi % 2 == 0, 0, 65535)[run]
        return d, 1.0 / 5000
    d = metres.astype(F32)
    if mode == "none":
        vals = np.array([0.0, -1.5, np.inf, -np.inf, 0.01, np.nextafter(F32(10), F32(np.inf))], F32)
        d = vals[(xi + 2 * yi) % len(vals)]
    elif mode == "holes":
        vals = np.array([np.nan, 0.0, -1.5, np.inf, -np.inf, 0.01, 10.0, np.nextafter(F32(10), F32(np.inf))], F32)
        sel = (xi + yi) % len(vals)
        d[hole] = vals[sel][hole]
        d[run] = np.array([0.0, np.inf, -2.0, 0.01], F32)[(xi + yi) % 4][run]
    return d, 1.0


def gpu_generate(pkg, torch, mapper, colors, depths, factor, poses, cap, pad=True):
    """B frames through generate_device out of padded, unaligned buffers -> (list of per-frame CLOUD arrays, counts)."""
    B = len(colors)
    h, w, ch = colors[0].shape
    es = depths[0].itemsize
    cs, ds = (w * ch + 5, w * es + 3 * es) if pad else (w * ch, w * es)
    cis, dis = (cs * h + 11, ds * h + 5 * es) if pad else (cs * h, ds * h)
    coff, doff = (3, es) if pad else (0, 0)
    cbuf = np.full(coff + cis * B + 16, 0xEE, np.uint8)
    dbuf = np.full(doff + dis * B + 16, 0xFF, np.uint8)
    for b in range(B):
        for r in range(h):
            cbuf[coff + b * cis + r * cs:][:w * ch] = colors[b][r].ravel()
            dbuf[doff + b * dis + r * ds:][:w * es] = depths[b][r].view(np.uint8)
    d_c, d_d = torch.from_numpy(cbuf).cuda(), torch.from_numpy(dbuf).cuda()
    pts = torch.full((B * cap * 16 + 16,), SENT, dtype=torch.uint8, device="cuda")
    cnt = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    dt = pkg.DEPTH_U16 if depths[0].dtype == np.uint16 else pkg.DEPTH_F32
    mapper.generate_device(d_d.data_ptr() + doff, dt, ds, dis, factor, d_c.data_ptr() + coff, ch, cs, cis, B, w, h,
                           CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], np.stack(poses), pts.data_ptr(), cap, cnt.data_ptr(), st)
    torch.cuda.synchronize()
    raw = pts.cpu().numpy()
    n = cnt.cpu().numpy()
    assert (raw[B * cap * 16:] == SENT).all()
    out = []
    for b in range(B):
        rows = raw[b * cap * 16:(b + 1) * cap * 16]
        assert 0 <= n[b] <= cap
        assert (rows[n[b] * 16:] == SENT).all(), "frame %d: rows past the count were written" % b
        out.append(rows[:n[b] * 16].view(pkg.CLOUD_DTYPE).copy())
    return out, n


def assert_same(got, ref, what=""):
    assert len(got) == len(ref), (what, len(got), len(ref))
    assert R.same_points(got, ref), what


# ---- generate

@pytest.mark.parametrize("step,kind,channels", [(1, "u16", 3), (2, "u16", 4), (3, "u16", 3), (1, "f32", 4), (2, "f32", 3), (3, "f32", 4)])
def test_generate_61x47_three_frames_three_poses(pkg, torch, step, kind, channels):
    """Padded, unaligned strides; holes of every kind, regular and in runs of more than 64 samples; one frame with no valid depth
    and one with every depth valid; three poses."""
    w, h, B = 61, 47, 3
    modes = ("holes", "none", "all")
    colors = [colour_image(w, h, channels, b) for b in range(B)]
    dd = [depth_image(w, h, kind, b, modes[b]) for b in range(B)]
    depths, factor = [d for d, _ in dd], dd[0][1]
    poses = [pose(b) for b in range(B)]
    m = pkg.CloudMapper(0.1, step, 200 + step)
    cap = m.capacity(w, h)
    assert cap == R.capacity(w, h, step)
    got, n = gpu_generate(pkg, torch, m, colors, depths, factor, poses, cap)
    refs = [R.generate(colors[b], depths[b], CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], poses[b], factor, step, 200 + step) for b in range(B)]
    assert len(refs[1]) == 0 and len(refs[2]) == cap and 0 < len(refs[0]) < cap
    if kind == "f32":
        assert np.isnan(refs[0]["x"]).any()   # a NaN depth is kept
    for b in range(B):
        assert_same(got[b], refs[b], "frame %d" % b)


def test_generate_f32_with_a_factor_and_identity_pose(pkg, torch):
    w, h = 61, 47
    color, (depth, _) = colour_image(w, h, 3), depth_image(w, h, "f32", 3)
    m = pkg.CloudMapper(0.1, 3, 0)
    got, _ = gpu_generate(pkg, torch, m, [color], [depth], 0.5, [np.eye(4)], m.capacity(w, h), pad=False)
    assert_same(got[0], R.generate(color, depth, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], np.eye(4), 0.5, 3, 0))


def test_generate_clamps_to_cap(pkg, torch):
    w, h, step = 61, 47, 2
    colors = [colour_image(w, h, 3, b) for b in range(2)]
    depths = [depth_image(w, h, "f32", 0, "all")[0], depth_image(w, h, "f32", 1, "holes")[0]]
    poses = [pose(1), pose(2)]
    m = pkg.CloudMapper(0.1, step, 255)
    refs = [R.generate(colors[b], depths[b], CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], poses[b], 1.0, step) for b in range(2)]
    cap = len(refs[1]) - 37
    assert 64 < cap < len(refs[1]) < len(refs[0])
    got, n = gpu_generate(pkg, torch, m, colors, depths, 1.0, poses, cap)
    assert list(n) == [cap, cap]
    for b in range(2):
        assert_same(got[b], refs[b][:cap], "frame %d" % b)


def test_generate_640x480_step_1_crosses_workgroups(pkg, torch):
    w, h, B = 640, 480, 2
    colors = [colour_image(w, h, 3, b) for b in range(B)]
    depths = [depth_image(w, h, "u16", b)[0] for b in range(B)]
    poses = [pose(0), pose(3)]
    m = pkg.CloudMapper(0.1, 1, 255)
    got, n = gpu_generate(pkg, torch, m, colors, depths, 1.0 / 5000, poses, w * h, pad=False)
    for b in range(B):
        ref = R.generate(colors[b], depths[b], CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], poses[b], 1.0 / 5000, 1)
        assert 1024 * 100 < len(ref) < w * h
        assert_same(got[b], ref, "frame %d" % b)


def test_generate_18_frames_18_poses(pkg, torch):
    """More frames than one launch carries poses for (16): every frame must meet its own pose."""
    w, h, B, step = 23, 17, 18, 2
    colors = [colour_image(w, h, 3, b) for b in range(B)]
    depths = [depth_image(w, h, "f32", b, "holes" if b % 3 else "all")[0] for b in range(B)]
    poses = [pose(b) for b in range(B)]
    m = pkg.CloudMapper(0.1, step, 255)
    got, n = gpu_generate(pkg, torch, m, colors, depths, 1.0, poses, m.capacity(w, h))
    for b in range(B):
        assert_same(got[b], R.generate(colors[b], depths[b], CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], poses[b], 1.0, step), "frame %d" % b)


# ---- voxel

def gpu_voxel(pkg, torch, mapper, clouds, cap=None, out_cap=None):
    """B clouds through voxel_device -> (list of per-frame outputs, counts); rows past a count must be untouched."""
    B = len(clouds)
    cap = cap or max(1, max(len(c) for c in clouds))
    out_cap = out_cap or cap
    buf = np.zeros((B, cap), pkg.CLOUD_DTYPE)
    buf["x"] = np.nan   # rows past a frame's count are not the filter's business
    for b, c in enumerate(clouds):
        buf[b, :len(c)] = c
    d_in = torch.from_numpy(buf.view(np.uint8).reshape(-1)).cuda()
    d_n = torch.from_numpy(np.array([len(c) for c in clouds], np.int32)).cuda()
    d_out = torch.full((B * out_cap * 16 + 16,), SENT, dtype=torch.uint8, device="cuda")
    d_on = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    mapper.voxel_device(d_in.data_ptr(), d_n.data_ptr(), B, cap, d_out.data_ptr(), out_cap, d_on.data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    raw, n = d_out.cpu().numpy(), d_on.cpu().numpy()
    assert (raw[B * out_cap * 16:] == SENT).all()
    assert (d_in.cpu().numpy() == buf.view(np.uint8).reshape(-1)).all(), "the input cloud was modified"
    out = []
    for b in range(B):
        rows = raw[b * out_cap * 16:(b + 1) * out_cap * 16]
        k = max(int(n[b]), 0)
        assert k <= out_cap and (rows[k * 16:] == SENT).all(), "frame %d: rows past the count were written" % b
        out.append(rows[:k * 16].view(pkg.CLOUD_DTYPE).copy())
    return out, n


@functools.lru_cache(maxsize=None)
def random_cloud(n, seed=0, side=8.0):
    """n points in a cube of `side` metres around a point off the origin (negative coordinates included), some rows non-finite."""
    rng = np.random.default_rng(1000 * seed + n)
    xyz = (rng.random((n, 3)) * side - [side * 0.4, side * 0.7, 1.0]).astype(F32)
    bad = rng.random(n) < 0.03
    if n > 1:
        xyz[bad, rng.integers(0, 3, bad.sum())] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), bad.sum())
    c = R.make_cloud(xyz, rng.integers(0, 256, (n, 4)))
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ref_voxel(n, seed, leaf):
    return R.voxel(random_cloud(n, seed), F32(leaf))


HAND = [
    (1.0, [[0.5, 0, 0], [-0.5, 0, 0]], None),                                      # floorf at negative coordinates
    (1.0, [[-0.25, -0.25, -0.25], [-0.75, -0.75, -0.75]], None),
    (0.5, [[1.0, 0, 0], [0.999, 0, 0], [0.5, 0, 0]], None),                        # a point on a cell face
    (1.0, [[0.1, 0.1, 0.1], [0.2, 0.2, 0.2]], [[255, 1, 0, 255], [254, 2, 0, 254]]),   # colour mean truncates
    (1.0, [[0.1, 0.1, 0.1], [np.nan, 0, 0], [0, np.inf, 0], [0.3, 0.3, 0.3], [0, 0, -np.inf]], [[10, 0, 0, 0]] * 5),
    (1.0, [[np.nan, 0, 0]], None),                                                 # none finite
    (1e-4, [[0, 0, 0], [10, 10, 10]], None),                                       # overflow: -1
    (1e-2, [[0, 0, 0], [10, 10, 10]], None),
    (1.0, [[1.5, 1.5, 1.5], [0.5, 1.5, 0.5], [1.5, 0.5, 0.5], [0.5, 0.5, 1.5], [0.5, 0.5, 0.5]], None),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_voxel_hand_cases(pkg, torch, case):
    leaf, xyz, rgba = HAND[case]
    c = R.make_cloud(xyz, rgba)
    ref, rn = R.voxel(c, F32(leaf))
    got, n = gpu_voxel(pkg, torch, pkg.CloudMapper(leaf, 3, 255), [c])
    assert n[0] == rn
    assert_same(got[0], ref)


def test_voxel_sum_is_sequential(pkg, torch):
    c, x = R.order_sensitive_cloud()
    got, n = gpu_voxel(pkg, torch, pkg.CloudMapper(1e5, 3, 255), [c])
    assert n[0] == 1
    assert got[0]["x"][0] == F32(R.seq_sum_f32(x) / F32(65)) != F32(R.pairwise_sum_f32(x) / F32(65))
    assert_same(got[0], R.voxel(c, F32(1e5))[0])


# leaf 4: 3 x 3 x 3 cells at most (idx < 8 bits, one radix pass); 0.25: two passes; 0.02 over the 8 m cube: 400^3 cells, idx beyond
# 24 bits, all four passes
@pytest.mark.parametrize("leaf", [4.0, 0.25, 0.02])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 40000])
def test_voxel_random_clouds(pkg, torch, n, leaf):
    c = random_cloud(n)
    ref, rn = ref_voxel(n, 0, leaf)
    if n == 40000:
        fin, idx, _ = R.voxel_indices(c, F32(leaf))
        assert (int(idx.max()) < 256) if leaf == 4.0 else (int(idx.max()) >= 1 << 24) if leaf == 0.02 else True
    got, gn = gpu_voxel(pkg, torch, pkg.CloudMapper(leaf, 3, 255), [c])
    assert gn[0] == rn
    assert_same(got[0], ref)


def test_voxel_batch_of_counts_0_1_40000(pkg, torch):
    leaf = 0.25
    clouds = [random_cloud(0), random_cloud(1, 1), random_cloud(40000)]
    got, n = gpu_voxel(pkg, torch, pkg.CloudMapper(leaf, 3, 255), clouds)
    refs = [R.voxel(clouds[0], F32(leaf)), R.voxel(clouds[1], F32(leaf)), ref_voxel(40000, 0, leaf)]
    assert list(n) == [0, refs[1][1], refs[2][1]]
    for b in range(3):
        assert_same(got[b], refs[b][0], "frame %d" % b)


def test_voxel_batch_whose_frames_need_different_pass_counts(pkg, torch):
    """A cloud a few centimetres across (idx in one byte) beside the 8 m cube (idx beyond 24 bits) at leaf 0.02: the batch runs four
    passes, the small frame's upper digits are all zero."""
    leaf = 0.02
    tiny = random_cloud(1025, 3).copy()
    for f in "xyz":
        tiny[f] = (tiny[f] * F32(0.01)).astype(F32)
    clouds = [tiny, random_cloud(40000), tiny[:65].copy()]
    _, idx, _ = R.voxel_indices(tiny, F32(leaf))
    assert int(idx.max()) < 256
    refs = [R.voxel(tiny, F32(leaf)), ref_voxel(40000, 0, leaf), R.voxel(clouds[2], F32(leaf))]
    got, n = gpu_voxel(pkg, torch, pkg.CloudMapper(leaf, 3, 255), clouds)
    assert list(n) == [r[1] for r in refs]
    for b in range(3):
        assert_same(got[b], refs[b][0], "frame %d" % b)


@pytest.mark.parametrize("leaf", [0.25, 0.02])
def test_voxel_frame_of_257_workgroups_beside_one(pkg, torch, leaf):
    """A frame of more than 256 workgroups: the scan of the per-workgroup counts goes a second round with a carry, and frame 1's rows
    of the per-workgroup counts and histograms sit 257 entries in."""
    clouds = [random_cloud((1 << 18) + 37), random_cloud(65, 1)]
    cap = max(len(c) for c in clouds)
    assert (cap + 1023) // 1024 == 257
    if leaf == 0.02:
        _, idx, _ = R.voxel_indices(clouds[0], F32(leaf))
        assert int(idx.max()) >= 1 << 24   # all four passes run
    refs = [R.voxel(c, F32(leaf)) for c in clouds]
    got, n = gpu_voxel(pkg, torch, pkg.CloudMapper(leaf, 3, 255), clouds)
    assert list(n) == [r[1] for r in refs]
    for b in range(2):
        assert_same(got[b], refs[b][0], "frame %d" % b)


def test_voxel_overflow_frame_beside_normal_frames(pkg, torch):
    leaf = 1e-4
    small = R.make_cloud((random_cloud(1025, 2)["x"][:, None] * [1, 0.5, 0.25] * F32(0.004)).astype(F32))   # a few centimetres across
    small = small[np.isfinite(small["x"])]
    wide = R.make_cloud([[0, 0, 0], [10, 10, 10], [1, 2, 3]])
    clouds = [small, wide, small[::-1].copy()]
    refs = [R.voxel(c, F32(leaf)) for c in clouds]
    assert refs[1][1] == -1 and refs[0][1] > 100 and refs[2][1] == refs[0][1]
    got, n = gpu_voxel(pkg, torch, pkg.CloudMapper(leaf, 3, 255), clouds)
    assert list(n) == [r[1] for r in refs]
    for b in (0, 2):
        assert_same(got[b], refs[b][0], "frame %d" % b)
    assert len(got[1]) == 0


def test_voxel_clamps_to_out_cap(pkg, torch):
    c = random_cloud(1025)
    ref, rn = ref_voxel(1025, 0, 0.25)
    assert rn > 300
    got, n = gpu_voxel(pkg, torch, pkg.CloudMapper(0.25, 3, 255), [c], out_cap=300)
    assert n[0] == 300
    assert_same(got[0], ref[:300])


# ---- end to end

@pytest.mark.parametrize("kind,channels", [("u16", 3), ("f32", 4)])
def test_keyframe_cloud_160x120(pkg, kind, channels):
    w, h = 160, 120
    color = colour_image(w, h, channels, 4)
    depth, factor = depth_image(w, h, kind, 2)
    M = pose(1)
    m = pkg.CloudMapper(0.1, 3, 255)
    for _ in range(2):   # (the second call runs on scratch that is already there)
        raw, out = m.keyframe_cloud(color, depth, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], M, factor)
        rraw = R.generate(color, depth, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], M, factor, 3, 255)
        rout, rn = R.voxel(rraw, F32(0.1))
        assert 10 < rn < len(rraw) < R.capacity(w, h, 3)
        assert_same(raw, rraw, "raw")
        assert_same(out, rout, "filtered")
    raw, out = m.keyframe_cloud(np.zeros((0, 0, 3), np.uint8), np.zeros((0, 0), F32), 1.0, 1.0, 0.0, 0.0, np.eye(4))
    assert len(raw) == 0 and len(out) == 0
