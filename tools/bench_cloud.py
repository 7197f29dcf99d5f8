"""Dense keyframe clouds (generatePointCloud + the voxel-grid filter; not the bench metric):
python tools/bench_cloud.py [--reps N] [--iters N]
  batched    B = 1 and B = 64 keyframes of 640x480 (U16 depth, 3-channel colour) in HBM, the reference's step 3 and leaf 0.1:
               generate = orbx_cloud_generate_device, voxel = orbx_cloud_voxel_device, both = one after the other
             device events around `iters` steps, warm-up first, the steps alternated `reps` times in one run; medians
  one frame  ms per call of orbx_keyframe_cloud (pageable host images in, host clouds out)
The first keyframe is checked against tests/cloud_ref.py before anything is timed.  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np   # noqa: E402
import torch         # noqa: E402

import cloud_ref as R  # noqa: E402

pkg = importlib.import_module("orb_slam2v2-1_amd")
FX, FY, CX, CY = 535.4, 539.2, 320.1, 247.6   # config/Asus.yaml
W, H, STEP, LEAF = 640, 480, 3, 0.1


def scene(k):
    """A room-like depth map (1 - 4.5 m, a step edge, 20 % holes) in millimetres * 5, and a colour image."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    metres = 1.0 + 2.0 * x / W + 0.8 * y / H + 0.7 * (x > W * (0.3 + 0.05 * (k % 8))) + 0.05 * np.sin(x * 0.07 + y * 0.05 + k)
    d = np.round(metres * 5000).astype(np.uint16)
    d[((x.astype(int) * 7 + y.astype(int) * 13) % 5) == 0] = 0
    c = np.stack([(x * 3 + y + k) % 256, (x + y * 5) % 256, (x * y + k) % 256], -1).astype(np.uint8)
    a = 0.05 * k
    M = np.eye(4)
    M[:3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
    M[:3, 3] = [0.1 * k, 0.0, 0.02 * k]
    return c, d, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    m = pkg.CloudMapper(LEAF, STEP, 255)
    cap = m.capacity(W, H)
    frames = [scene(k) for k in range(64)]
    c0, d0, M0 = frames[0]
    raw, out = m.keyframe_cloud(c0, d0, FX, FY, CX, CY, M0, 1.0 / 5000)
    rraw = R.generate(c0, d0, FX, FY, CX, CY, M0, 1.0 / 5000, STEP, 255)
    rout, _ = R.voxel(rraw, np.float32(LEAF))
    res = {"workload": "640x480 keyframes, U16 depth, 3-channel colour, step %d, leaf %g" % (STEP, LEAF),
           "equals_numpy": bool(R.same_points(raw, rraw) and R.same_points(out, rout)),
           "points_per_keyframe": len(raw), "voxels_per_keyframe": len(out)}
    st = torch.cuda.current_stream().cuda_stream

    def timed(f, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    for B in (1, 64):
        d_c = torch.from_numpy(np.stack([f[0] for f in frames[:B]])).cuda()
        d_d = torch.from_numpy(np.stack([f[1] for f in frames[:B]])).cuda()
        T = np.stack([f[2] for f in frames[:B]])
        pts = torch.zeros((B, cap, 16), dtype=torch.uint8, device="cuda")
        vox = torch.zeros((B, cap, 16), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
        vcnt = torch.zeros(B, dtype=torch.int32, device="cuda")

        def generate():
            m.generate_device(d_d.data_ptr(), pkg.DEPTH_U16, W * 2, W * H * 2, 1.0 / 5000, d_c.data_ptr(), 3, W * 3, W * H * 3, B, W, H,
                              FX, FY, CX, CY, T, pts.data_ptr(), cap, cnt.data_ptr(), st)

        def voxel():
            m.voxel_device(pts.data_ptr(), cnt.data_ptr(), B, cap, vox.data_ptr(), cap, vcnt.data_ptr(), st)

        def both():
            generate()
            voxel()

        for f in (generate, voxel, both):
            timed(f, 5)
        t = {"generate": [], "voxel": [], "both": []}
        for _ in range(a.reps):
            t["generate"].append(timed(generate, a.iters))
            t["voxel"].append(timed(voxel, a.iters))
            t["both"].append(timed(both, a.iters))
        med = {k: float(np.median(v)) for k, v in t.items()}
        res["B%d" % B] = {"generate_ms": med["generate"], "voxel_ms": med["voxel"], "both_ms": med["both"],
                          "keyframes_per_s": B / med["both"] * 1e3, "points": int(cnt.sum().item()), "voxels": int(vcnt.sum().item()),
                          "spread": {k: [float(min(v)), float(max(v))] for k, v in t.items()}}

    def per_call(f, n=30, warm=5):
        for _ in range(warm):
            f()
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        return (time.perf_counter() - t0) / n * 1e3
    res["keyframe_cloud_ms"] = float(np.median([per_call(lambda: m.keyframe_cloud(c0, d0, FX, FY, CX, CY, M0, 1.0 / 5000))
                                                for _ in range(a.reps)]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
