"""One Sim3Solver call for all loop candidates of a LoopClosing::ComputeSim3 (orbs_sim3_ransac_batch, k_sim3_prepare / k_sim3_ransac /
k_sim3_select): 4 candidates x 300 iterations x 100 pairs by default.

  python tools/bench_sim3.py                     # 200 timed calls after 20 warm-ups
  python tools/bench_sim3.py 8 300 200           # candidates, iterations, pairs
  rocprofv3 --kernel-trace --stats -- python tools/bench_sim3.py       # the three kernels apart

Scene: tests/sim3_scene.py (depth 3-9, 30 % gross outliers, noise 0.01 z / 5, rotation 0.2 rad), one seed per candidate.  The
figure is a host clock around the synchronous call on host arrays - pairs and sets up, three launches, counts, models and all
flags down - the median of the timed calls: what the loop-closing thread waits.  The reference's own Sim3Solver needs OpenCV and
cannot be built beside it, so there is no ratio.
"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3_scene as S        # noqa: E402

a = [int(x) for x in sys.argv[1:]]
B, its, n = (a + [4, 300, 100][len(a):])[:3]
scs = [S.make(100 + b, n, iterations=its) for b in range(B)]
pkg = importlib.import_module("orb_slam2v2-1_amd")
off, soff = np.arange(B + 1) * n, np.arange(B + 1) * its
pairs, sets = np.concatenate([s["pairs"] for s in scs]), np.concatenate([s["sets"] for s in scs])
problems = np.concatenate([S.problem(s) for s in scs])
WARM, CALLS = 20, 200
ms = []
for i in range(WARM + CALLS):
    t0 = time.perf_counter()
    out = pkg.sim3_ransac_batch(pairs, off, problems, sets, soff)
    ms.append((time.perf_counter() - t0) * 1e3)
ms = np.array(ms[WARM:])
print("%d candidates x %d iterations x %d pairs: hit iterations %s, inliers %s | host clock around the batched call: median %.3f ms "
      "(min %.3f, p90 %.3f)" % (B, its, n, [o["hit_iteration"] for o in out], [o["best_inliers"] for o in out], np.median(ms), ms.min(),
                                np.percentile(ms, 90)), flush=True)
