"""One Initializer::Initialize call (orbi_initialize*, k_init_normalize / k_init_ransac / k_init_select / k_init_reconstruct) at N
matches and 200 iterations.

  python tools/bench_initializer.py 100 500 2000         # match counts; 200 timed calls after 20 warm-ups each
  rocprofv3 --kernel-trace --stats -- python tools/bench_initializer.py 500       # the four kernels apart
  python tools/bench_initializer.py --pack DIR 100 500 2000                       # only write DIR/init_N.bin, the input of
                                                                                  # tests/cpp/initializer_lockstep.cc (its third
                                                                                  # argument repeats the chain and prints s / run)

Scene: tests/init_scene.py (640x480, 0.5 px noise, 20 % gross outliers, baseline 0.3 at depth 2-8, 5 degrees).  Two figures per
size, each the median of the timed calls: HIP events on the stream around the device form (orbi_initialize_device: matches and
sets up, four launches, results down - what the GPU spends), and a host clock around the synchronous host-array call (what the
caller waits, the key arrays' upload and the runtime's calls included).  The reference's own Initializer needs OpenCV and cannot
be built beside it; the CPU figure of profiles/README.md is the lockstep build of the kernels' text on one core.
"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import init_scene as S        # noqa: E402

args = sys.argv[1:]
pack = None
if args[:1] == ["--pack"]:
    pack, args = args[1], args[2:]
sizes = [int(a) for a in args] or [100, 500, 2000]
scenes = {n: S.make(n, n, outliers=n // 5, iterations=200) for n in sizes}
if pack:
    os.makedirs(pack, exist_ok=True)
    for n, sc in scenes.items():
        open(os.path.join(pack, "init_%d.bin" % n), "wb").write(S.pack(sc))
    sys.exit(0)

import torch                  # noqa: E402
pkg = importlib.import_module("orb_slam2v2-1_amd")
WARM, CALLS = 20, 200
for n, sc in scenes.items():
    ini = pkg.Initializer(sc["keys1"], sc["K4"], iterations=200)
    recs = []
    for k in (sc["keys1"], sc["keys2"]):
        kp = np.zeros(len(k), pkg.KP_DTYPE)
        kp["x"], kp["y"] = k[:, 0], k[:, 1]
        recs.append(torch.from_numpy(kp.view(np.uint8).copy()).cuda())
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    dargs = (recs[0].data_ptr(), n, recs[1].data_ptr(), n, sc["matches"], sc["sets"], sc["K4"])
    host = ini.initialize(sc["keys2"], sc["matches"], sc["sets"])
    dev = pkg.initialize_device(*dargs, stream=stream)
    assert host[0] == dev[0] and host[1].tobytes() == dev[1].tobytes() and host[3].tobytes() == dev[3].tobytes()
    ev_ms, host_ms = [], []
    for i in range(WARM + CALLS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pkg.initialize_device(*dargs, stream=stream)
        b.record(); b.synchronize()
        ev_ms.append(a.elapsed_time(b))
    for i in range(WARM + CALLS):
        t0 = time.perf_counter()
        ini.initialize(sc["keys2"], sc["matches"], sc["sets"])
        host_ms.append((time.perf_counter() - t0) * 1e3)
    ev_ms, host_ms = np.array(ev_ms[WARM:]), np.array(host_ms[WARM:])
    info = host[5]
    print("N %d: result %s, model %d, inliers %s, ngood %s | device form, HIP events: median %.3f ms (min %.3f, p90 %.3f) | host form, host "
          "clock: median %.3f ms (min %.3f, p90 %.3f)" % (n, host[0], info["model"], list(info["inliers"]), list(info["ngood"]), np.median(ev_ms),
                                                         ev_ms.min(), np.percentile(ev_ms, 90), np.median(host_ms), host_ms.min(),
                                                         np.percentile(host_ms, 90)), flush=True)
