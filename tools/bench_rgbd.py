"""RGB-D front end against the gray mono step (not the bench metric): python tools/bench_rgbd.py [--reps N] [--iters N]
  batched  640x480 x 64 images, config/Asus.yaml settings (1000 features, 1.2, 8 levels, 20 / 7), inputs in HBM:
             mono  = orbx_extract_batch_device on gray images
             rgbd  = orbx_gray_from_color_device (BGR) + orbx_extract_batch_device + orbm_rgbd_batch_device (CV_16U depth, 1/5000)
           device events around `iters` steps, warm-up first, the two steps alternated `reps` times in one run
  one frame  ms per call of orbx_rgbd_frame (colour + depth from host memory) against orbx_extract (gray) on the same frame
Prints one JSON line."""
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

import rgbd_ref as R  # noqa: E402

pkg = importlib.import_module("orb_slam2v2-1_amd")
synth = importlib.import_module("orb_slam2v2-1_amd.synth")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cam", default="asus", choices=["asus", "tum1"])
    a = ap.parse_args()
    w, h, B = 640, 480, 64
    cam = pkg.RGBDCamera(**(R.ASUS if a.cam == "asus" else R.TUM1))
    grays = np.stack([synth.frame(w, h, i % 16) for i in range(B)])
    g = grays.astype(np.int32)
    colors = np.stack([g, (3 * g) // 4 + 40, 255 - g // 2], -1).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    depth1 = np.round((1.0 + 1.5 * x / w + 0.7 * y / h) * 5000).astype(np.uint16)
    depths = np.stack([depth1] * B)
    ex = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    ex(grays[0])
    cap = ex.max_keypoints()
    d_gray_in = torch.from_numpy(grays).cuda()
    d_col = torch.from_numpy(colors).cuda()
    d_dep = torch.from_numpy(depths).cuda()
    d_gray = torch.zeros((B, h, w), dtype=torch.uint8, device="cuda")
    kps = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    kun = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    ur = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    dp = torch.zeros((B, cap), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def mono():
        ex.extract_batch_device(d_gray_in.data_ptr(), B, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), cap, st)

    def rgbd():
        pkg.gray_from_color_device(d_col.data_ptr(), B, w, h, 3, False, w * 3, w * h * 3, d_gray.data_ptr(), w, w * h, st)
        ex.extract_batch_device(d_gray.data_ptr(), B, w, h, w, w * h, kps.data_ptr(), desc.data_ptr(), cnt.data_ptr(), cap, st)
        pkg.rgbd_batch_device(kps.data_ptr(), cnt.data_ptr(), B, cap, d_dep.data_ptr(), pkg.DEPTH_U16, w, h, w * 2, w * h * 2, 1.0 / 5000,
                              cam, kun.data_ptr(), ur.data_ptr(), dp.data_ptr(), st)

    def gray_only():
        pkg.gray_from_color_device(d_col.data_ptr(), B, w, h, 3, False, w * 3, w * h * 3, d_gray.data_ptr(), w, w * h, st)

    def timed(f, iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters

    for f in (mono, rgbd, gray_only):
        timed(f, 5)
    res = {"mono": [], "rgbd": [], "gray_kernel": []}
    for _ in range(a.reps):
        res["mono"].append(timed(mono, a.iters))
        res["rgbd"].append(timed(rgbd, a.iters))
        res["gray_kernel"].append(timed(gray_only, a.iters))
    med = {k: float(np.median(v)) for k, v in res.items()}
    out = {"workload": "640x480 x %d, 1000 features, 1.2, 8, 20/7, cam %s" % (B, a.cam),
           "mono_ms": med["mono"], "rgbd_ms": med["rgbd"], "gray_kernel_ms": med["gray_kernel"],
           "mono_images_per_s": B / med["mono"] * 1e3, "rgbd_images_per_s": B / med["rgbd"] * 1e3,
           "rgbd_over_mono": med["mono"] / med["rgbd"],
           "spread": {k: [float(min(v)), float(max(v))] for k, v in res.items()}}
    # one frame from host memory: the reference's call shape
    ex1 = pkg.ORBextractor(1000, 1.2, 8, 20, 7)
    c0, d0, g0 = colors[0], depths[0], grays[0]

    def per_call(f, n=50, warm=5):
        for _ in range(warm):
            f()
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        return (time.perf_counter() - t0) / n * 1e3
    t_ex, t_rgbd = [], []
    for _ in range(a.reps):
        t_ex.append(per_call(lambda: ex1(g0)))
        t_rgbd.append(per_call(lambda: ex1.rgbd_frame(c0, d0, cam, 1.0 / 5000, rgb=False)))
    out["orbx_extract_ms"] = float(np.median(t_ex))
    out["orbx_rgbd_frame_ms"] = float(np.median(t_rgbd))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
