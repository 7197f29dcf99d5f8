"""One PnPsolver::iterate call for all candidates of a Tracking::Relocalization pass (orbp_pnp_ransac_batch, k_pnp_ransac /
k_pnp_refine / k_pnp_select): 4 candidates x 35 iterations x 100 correspondences by default, Relocalization's shape.

  python tools/bench_pnp.py                      # 200 timed calls after 20 warm-ups
  python tools/bench_pnp.py 8 35 200             # candidates, iterations, correspondences
  rocprofv3 --kernel-trace --stats -- python tools/bench_pnp.py        # the three kernels apart

Scene: tests/pnp_scene.py (depth 3-9, 30 % gross outliers, half a pixel of noise at level 0), one seed per candidate.  The figure
is a host clock around the synchronous call on host arrays - correspondences and sets up, three launches, counts, models, poses
and all flags down - the median of the timed calls: what the tracking thread waits.  The reference's own PnPsolver needs OpenCV's
legacy C API and cannot be built beside it, so there is no ratio.
"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnp_scene as S         # noqa: E402

a = [int(x) for x in sys.argv[1:]]
B, its, n = (a + [4, 35, 100][len(a):])[:3]
b = S.pack_scenes([S.make(100 + k, n, iterations=its) for k in range(B)])
pkg = importlib.import_module("orb_slam2v2-1_amd")
WARM, CALLS = 20, 200
ms = []
for i in range(WARM + CALLS):
    t0 = time.perf_counter()
    out = pkg.pnp_ransac_batch(b["corrs"], b["offsets"], b["problems"], b["sets"], b["set_offsets"])
    ms.append((time.perf_counter() - t0) * 1e3)
ms = np.array(ms[WARM:])
print("%d candidates x %d iterations x %d correspondences: hit iterations %s, refined inliers %s | host clock around the batched call: "
      "median %.3f ms (min %.3f, p90 %.3f)" % (B, its, n, [o["hit_iteration"] for o in out], [o["refined_inliers"] for o in out],
                                               np.median(ms), ms.min(), np.percentile(ms, 90)), flush=True)
