"""One Optimizer::LocalBundleAdjustment call (orbb_local_bundle_adjustment, the k_lba_* kernels under their host driver) at 10 / 20 / 40
free keyframes with 1000 / 2000 / 4000 points.

  python tools/bench_lba.py                      # the three sizes; 20 timed calls after 5 warm-ups each
  python tools/bench_lba.py 10:1000 40:4000      # free keyframes : points
  rocprofv3 --kernel-trace --stats -- python tools/bench_lba.py 20:2000          # the kernels apart
  python tools/bench_lba.py --pack DIR           # only write DIR/lba_K_P.bin, the input of tests/cpp/lba_lockstep.cc
  python tools/bench_lba.py --lockstep EXE       # time that program on the same scenes instead: the kernels' text on ONE host core

Scene: tests/lba_scene.py (KITTI-00 camera, half the observations stereo, 0.7 px noise scaled by the level, 5 % gross outliers, four
fixed keyframes beside the free ones).  The figure is the median of a host clock around the synchronous call, which ends in a stream
synchronisation: what the mapping thread waits, staging, the per-trial synchronisations and the runtime's calls included.  The call
owns its stream, so no event of the caller brackets it; the kernels' own time is the rocprofv3 run's.  Passes, launches and
synchronisations per call are counted from the call's own record (iterations and trials per round) by the rule of DESIGN.md section
6.  There is no g2o build on this hardware: no speed-up is claimed."""
import importlib
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lba_scene as S        # noqa: E402

args = sys.argv[1:]
pack = lockstep = None
if args[:1] == ["--pack"]:
    pack, args = args[1], args[2:]
if args[:1] == ["--lockstep"]:
    lockstep, args = args[1], args[2:]
sizes = [tuple(int(x) for x in a.split(":")) for a in args] or [(10, 1000), (20, 2000), (40, 4000)]
WARM, CALLS = 5, 20
pkg = importlib.import_module("orb_slam2v2-1_amd")


def packed(sc):
    sched = pkg.lba_schedule()
    return (np.array([len(sc["kfs"]), len(sc["pts"]), len(sc["obs"]), 0], np.int32).tobytes() + sched.tobytes() + sc["kfs"].tobytes() +
            sc["pts"].tobytes() + sc["obs"].tobytes())


def counts(info, nf):
    """-> (passes over the edges, launches, synchronisations) of one call: per linearisation 4 launches (3 without a free pose), per
    trial 6 (5), per round the table (a fill and a launch), the two classifications, the first and the last kernel"""
    its, trs = sum(info["iterations"]), sum(info["trials"])
    rounds_run = sum(1 for i in info["iterations"] if i)
    launches = 2 + its * (4 if nf else 3) + trs * (6 if nf else 5) + (2 * rounds_run if nf else 0) + 2
    syncs = trs + rounds_run + 1 + 1      # every trial, the first linearisation of a round, the flags between the rounds, the results
    return its + trs + 2, launches, syncs


for nfree, npts in sizes:
    sc = S.make(seed=900 + nfree, nfree=nfree, nfixed=4, npts=npts, stereo=0.5, outliers=0.05)
    K, P, E = len(sc["kfs"]), len(sc["pts"]), len(sc["obs"])
    if pack:
        os.makedirs(pack, exist_ok=True)
        open(os.path.join(pack, "lba_%d_%d.bin" % (nfree, npts)), "wb").write(packed(sc))
        continue
    if lockstep:
        with tempfile.TemporaryDirectory() as d:
            open(os.path.join(d, "in.bin"), "wb").write(packed(sc))
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                subprocess.run([lockstep, os.path.join(d, "in.bin"), os.path.join(d, "out.bin")], check=True)
                t.append(time.perf_counter() - t0)
        print("lockstep %d free keyframes, %d points, %d observations: %.1f ms (median of 3 runs of the program, one host core)" % (
            nfree, P, E, 1e3 * float(np.median(t))))
        continue
    ms = []
    for i in range(WARM + CALLS):
        t0 = time.perf_counter()
        res = pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"])
        ms.append(1e3 * (time.perf_counter() - t0))
    info = res[3]
    passes, launches, syncs = counts(info, info["free_poses"][0])
    print("%d free keyframes (%d in all), %d points, %d observations: %.2f ms median, %.2f ms min over %d calls | iterations %s trials %s erased %d | "
          "%d passes over the edges, %d launches, %d synchronisations" % (nfree, K, P, E, float(np.median(ms[WARM:])), min(ms[WARM:]), CALLS,
                                                                          info["iterations"], info["trials"], info["erased"], passes, launches, syncs))
