"""One Optimizer::OptimizeSim3 call (orbz_optimize_sim3*, k_sim3_opt): wall time of the synchronous host-array call, which ends in the
stream synchronisation - one upload, one launch, one download.

  python tools/bench_sim3opt.py                  # out65, 300 matches, a batch of 8 x 300 against 8 single calls; 300 timed calls after 30 warm-ups
  rocprofv3 --kernel-trace --stats -- python tools/bench_sim3opt.py       # k_sim3_opt alone

Scenes: tests/sim3opt_scene.py (KITTI-00 intrinsics, 20 % gross outliers, a start 0.025 rad / 4 cm / 1.5 % off).  Per figure the
median, the minimum and the 10th / 90th percentile of the timed calls; the batch and the 8 single calls alternate inside one loop,
so that both see the same machine.  The last line is the same row set through the numpy restatement tests/sim3opt_ref.py on the
host - for scale only: it is a test reference, not an implementation anybody would run.  There is no g2o build on this hardware to
set beside either.
"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sim3opt_ref as R        # noqa: E402
import sim3opt_scene as S      # noqa: E402
pkg = importlib.import_module("orb_slam2v2-1_amd")

WARM, CALLS = 30, 300


def stats(ms):
    ms = np.array(ms[WARM:])
    return "median %.3f ms (min %.3f, p10 %.3f, p90 %.3f, %d calls)" % (np.median(ms), ms.min(), np.percentile(ms, 10), np.percentile(ms, 90), len(ms))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


cases = {"out65": S.case("out65"), "n300": S.make(seed=301, n=300, outliers=0.2)}
for name, sc in cases.items():
    m, pr = sc["matches"], sc["prob"]
    T, dr, ni, info = pkg.optimize_sim3(m, pr)
    ms = [timed(lambda: pkg.optimize_sim3(m, pr)) for _ in range(WARM + CALLS)]
    print("%s: %d matches, %d inliers, iterations %s, trials %s | one call, host clock: %s" % (name, len(m), ni, info["iterations"], info["trials"],
                                                                                        stats(ms)), flush=True)

scs = [S.make(seed=310 + b, n=300, outliers=0.2) for b in range(8)]
mm = np.concatenate([s["matches"] for s in scs])
off = np.arange(9, dtype=np.int32) * 300
probs = np.array([s["prob"] for s in scs])
batch = pkg.optimize_sim3_batch(mm, off, probs)
for b, s in enumerate(scs):
    one = pkg.optimize_sim3(s["matches"], s["prob"])
    assert one[0].tobytes() == batch[0][b].tobytes() and (one[1] == batch[1][off[b]:off[b + 1]]).all() and one[2] == batch[2][b]
bt, st = [], []
for _ in range(WARM + CALLS):
    bt.append(timed(lambda: pkg.optimize_sim3_batch(mm, off, probs)))
    st.append(timed(lambda: [pkg.optimize_sim3(s["matches"], s["prob"]) for s in scs]))
print("8 problems x 300 matches | one batch call: %s | 8 single calls: %s" % (stats(bt), stats(st)), flush=True)

sc = cases["n300"]
rt = [timed(lambda: R.optimize_sim3(sc["matches"], sc["prob"])) for _ in range(20)]
print("n300 through tests/sim3opt_ref.py (numpy, one host thread; for scale only): median %.1f ms (min %.1f, %d calls)" % (np.median(rt), min(rt), len(rt)))
