"""One Optimizer::PoseOptimization call (orbo_pose_optimization*, k_pose_opt) at n edges.

  python tools/bench_poseopt.py 300 1000 2000            # edge counts; 200 timed calls after 20 warm-ups each
  rocprofv3 --kernel-trace --stats -- python tools/bench_poseopt.py 1000        # k_pose_opt alone

Scene: tests/pose_scene.py (KITTI-00 intrinsics, 30 % monocular entries, 20 % gross outliers, the motion-model guess ~0.01 rad /
0.15 m off).  Two figures per size, each the median of the timed calls: HIP events on the stream around the device form
(orbo_pose_optimization_device: the 16-byte map-point records up, the one launch, flags / pose / info down - what the GPU spends),
and a host clock around the synchronous host-array call (what the caller waits, PCIe and the runtime's calls included).
There is no g2o build on this hardware to set beside either.
"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch                  # noqa: E402
import pose_scene as S        # noqa: E402
pkg = importlib.import_module("orb_slam2v2-1_amd")

WARM, CALLS = 20, 200
for n in [int(a) for a in sys.argv[1:]] or [300, 1000, 2000]:
    sc = S.make(n, n, mono=0.3, outliers=0.2)
    obs, cam, T0 = sc["obs"], pkg.Camera(*S.CAM), sc["Tcw0"]
    kun = np.zeros(n, pkg.KP_DTYPE)
    kun["x"], kun["y"], kun["octave"] = obs["u"], obs["v"], sc["octave"]
    pts = np.zeros(n, pkg.POSE_WORLDPOS_DTYPE)
    for f in ("valid", "wx", "wy", "wz"):
        pts[f] = obs[f]
    d_kun = torch.from_numpy(kun.view(np.uint8)).cuda()
    d_ur = torch.from_numpy(obs["ur"].copy()).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    host = pkg.pose_optimization(obs, cam, T0)
    dev = pkg.pose_optimization_device(d_kun.data_ptr(), d_ur.data_ptr(), n, S.INV_SIGMA2, pts, cam, T0, stream=stream)
    assert host[0].tobytes() == dev[0].tobytes() and (host[1] == dev[1]).all() and host[2] == dev[2]
    ev_ms, host_ms = [], []
    for i in range(WARM + CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pkg.pose_optimization_device(d_kun.data_ptr(), d_ur.data_ptr(), n, S.INV_SIGMA2, pts, cam, T0, stream=stream)
        b.record(); b.synchronize()
        ev_ms.append(a.elapsed_time(b))
    for i in range(WARM + CALLS):
        t0 = time.perf_counter()
        pkg.pose_optimization(obs, cam, T0)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    ev_ms, host_ms = np.array(ev_ms[WARM:]), np.array(host_ms[WARM:])
    info = host[3]
    print("n %d: ngood %d, iterations %s, trials %s | device form, HIP events: median %.3f ms (min %.3f, p90 %.3f) | host form, host clock: "
          "median %.3f ms (min %.3f, p90 %.3f)" % (n, host[2], info["iterations"], info["trials"], np.median(ev_ms), ev_ms.min(),
                                                  np.percentile(ev_ms, 90), np.median(host_ms), host_ms.min(), np.percentile(host_ms, 90)), flush=True)
