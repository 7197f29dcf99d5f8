"""One Optimizer::OptimizeEssentialGraph call (orbg_optimize_essential_graph, the k_eg_* kernels under their host driver) on a synthetic
trajectory with one loop, at the density of the ring scenes of tests/essential_scene.py: a spanning-tree chain, covisibility edges
to the two keyframes before the parent (band 3), the last five keyframes carrying a CorrectedSim3, six loop connections from the
last two keyframes to the first three, fixed scale, two map points per keyframe.

  python tools/bench_essential.py                # 250 and 1000 keyframes
  python tools/bench_essential.py 1000 2000      # keyframes
  rocprofv3 --kernel-trace --stats -- python tools/bench_essential.py 1000          # the kernels apart

The figure is the median of a host clock around the synchronous call, which ends in a stream synchronisation: what the loop-closing
thread waits, the host's symbolic factorisation, staging, the per-trial synchronisations and the runtime's calls included.  Blocks,
levels and launches are the call's own record (info).  The time per linearisation and per trial (assemble, factorise, the two
substitutions, update, evaluate: "a solve") is a least-squares fit of  time = fixed + iterations * linearisation + trials * solve
over calls limited to 1, 2, 3 and 20 iterations, whose (iterations, trials) are not collinear as soon as an iteration rejects a
trial; where they are collinear the two are reported together.  There is no g2o build on this hardware: no speed-up is claimed."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import essential_scene as S        # noqa: E402

sizes = [int(a) for a in sys.argv[1:]] or [250, 1000]
WARM, CALLS = 1, 5
pkg = importlib.import_module("orb_slam2v2-1_amd")

for n in sizes:
    sc = S.make(**S._ring(n, 3, 900 + n, True, rot=0.002, trans=0.005))
    rows = []
    for its in (1, 2, 3, 20):
        ms = []
        for i in range(WARM + CALLS):
            t0 = time.perf_counter()
            res = pkg.optimize_essential_graph(sc["vertices"], sc["edges"], sc["points"], True, iterations=its)
            ms.append(1e3 * (time.perf_counter() - t0))
        info = res[3]
        rows.append((info["iterations"], info["trials"], float(np.median(ms[WARM:])), min(ms[WARM:]), info))
    info = rows[-1][4]
    print("%d keyframes, %d edges, %d points: %.1f ms median, %.1f ms min over %d calls | iterations %d trials %s end %d chi2 %.3e -> %.3e | "
          "%d free vertices, %d factor blocks, %d levels, %d launches, %d synchronisations" % (
              n, len(sc["edges"]), len(sc["points"]), rows[-1][2], rows[-1][3], CALLS, info["iterations"], info["trials_it"][:info["iterations"]],
              info["end"], info["chi2_first"], info["chi2_last"], info["free_vertices"], info["blocks"], info["levels"], info["launches"],
              info["trials"] + 1))
    A = np.array([[1.0, r[0], r[1]] for r in rows])
    y = np.array([r[2] for r in rows])
    if np.linalg.matrix_rank(A) == 3:
        fixed, lin, solve = np.linalg.lstsq(A, y, rcond=None)[0]
        print("    fit over (iterations, trials, ms) = %s: fixed %.2f ms, one linearisation %.2f ms, one solve %.2f ms (%.1f us per launch of its %d)" % (
            [(r[0], r[1], round(r[2], 1)) for r in rows], fixed, lin, solve, 1e3 * solve / (4 + 3 * info["levels"]), 4 + 3 * info["levels"]))
    else:
        fixed, both = np.linalg.lstsq(A[:, :2], y, rcond=None)[0]
        print("    (iterations, trials, ms) = %s are collinear: fixed %.2f ms, one linearisation and one solve together %.2f ms" % (
            [(r[0], r[1], round(r[2], 1)) for r in rows], fixed, both))
