"""The occupancy octree of a synthetic room-like shell (orbx_octree_device): device events around `reps` calls, then one host call.

  python tools/bench_octomap.py 1000000 10x8x3 20        # points, box in metres, timed calls
  rocprofv3 --kernel-trace --stats -- python tools/bench_octomap.py 1000000 10x8x3 10     # per-kernel times (profiles/README.md)
"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("orb_slam2v2-1_amd")
import torch

def shell(n, size, seed=1):
    """n points on the six faces of a box of `size` metres centred on the origin, 1 cm of noise along the normal."""
    rng = np.random.default_rng(seed)
    sx, sy, sz = size
    areas = np.array([sy * sz, sy * sz, sx * sz, sx * sz, sx * sy, sx * sy])
    face = rng.choice(6, n, p=areas / areas.sum())
    p = (rng.random((n, 3)) - 0.5) * np.array(size)
    ax = face // 2
    p[np.arange(n), ax] = np.where(face % 2 == 0, -0.5, 0.5) * np.array(size)[ax] + rng.normal(0, 0.01, n)
    return p.astype(np.float32)

n, size, reps = int(sys.argv[1]), [float(v) for v in sys.argv[2].split("x")], int(sys.argv[3])
pts = np.zeros(n, pkg.CLOUD_DTYPE)
xyz = shell(n, size)
pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
m = pkg.CloudMapper(0.1, 3, 255)
d_in = torch.from_numpy(pts.view(np.uint8).reshape(-1)).cuda()
d_n = torch.tensor([n], dtype=torch.int32, device="cuda")
cap_d, cap_l = 64 << 20, 4 << 20
d_data = torch.zeros(cap_d, dtype=torch.uint8, device="cuda")
d_leaf = torch.zeros(cap_l * 8, dtype=torch.uint8, device="cuda")
d_info = torch.zeros(56, dtype=torch.uint8, device="cuda")
st = torch.cuda.current_stream().cuda_stream
def call():
    m.octree_device(d_in.data_ptr(), d_n.data_ptr(), 1, n, None, 0.1, d_data.data_ptr(), cap_d, d_leaf.data_ptr(), cap_l, d_info.data_ptr(), st)
call(); torch.cuda.synchronize()
info = pkg.OctreeInfo.from_buffer_copy(d_info.cpu().numpy().tobytes()).as_dict()
print("n", n, "box", size, info, flush=True)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
ev[0].record()
for i in range(reps):
    call(); ev[i + 1].record()
torch.cuda.synchronize()
ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]
print("ms per call:", " ".join("%.3f" % v for v in ms), "| median %.3f" % float(np.median(ms)), flush=True)
t0 = time.perf_counter()
file, hinfo = m.octomap_bt(pts)
print("host form (PCIe both ways): %.1f ms, %d bytes" % ((time.perf_counter() - t0) * 1e3, len(file)), flush=True)
