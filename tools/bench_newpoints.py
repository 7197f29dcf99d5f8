"""LocalMapping::CreateNewMapPoints on the device (orbl_triangulate, orbl_create_new_map_points; k_new_points): wall time of the
synchronous host-array calls, each of which ends in its stream synchronisation.

  python tools/bench_newpoints.py                # 100 timed calls after 10 warm-ups per figure
  rocprofv3 --kernel-trace --stats -- python tools/bench_newpoints.py       # k_new_points, k_tri_match and the rest alone

Figures: (1) one orbl_triangulate of 300 matches; (2) the chain for 10 neighbours (stereo rule) and for 20 (monocular rule) of a
current keyframe with 2000 features: ONE call, the flags updated on the device; (3) the same work as a host loop over the two entry
points, orbm_search_for_triangulation + orbl_triangulate per neighbour with the flags updated on the host in between - what a caller
had to do before the chain existed.  (2) and (3) alternate inside one loop, so that both see the same machine, and are checked
byte-equal first.  Scenes: tests/newpoints_scene.py.  Per figure the median, the minimum and the 10th / 90th percentile.
"""
import importlib, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import newpoints_scene as S      # noqa: E402
pkg = importlib.import_module("orb_slam2v2-1_amd")

WARM, CALLS = 10, 100


def stats(ms):
    ms = np.array(ms[WARM:])
    return "median %.3f ms (min %.3f, p10 %.3f, p90 %.3f, %d calls)" % (np.median(ms), ms.min(), np.percentile(ms, 10), np.percentile(ms, 90), len(ms))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def kf_of(k):
    return pkg.newpoints_keyframe(k["view"], k["kp"], k["st"], k["sf"], k["sig2"])


sc = S.make(300, 300, "mixed", "mixed")
a, b = kf_of(sc["kf1"]), kf_of(sc["kf2"])
pts, nnew = pkg.triangulate_new_points(a, b, sc["pairs"])
ms = [timed(lambda: pkg.triangulate_new_points(a, b, sc["pairs"])) for _ in range(WARM + CALLS)]
print("orbl_triangulate, 300 matches (%d accepted) | one call, host clock: %s" % (nnew, stats(ms)), flush=True)

for nn, mono in ((10, False), (20, True)):
    ang = np.linspace(0, 2 * np.pi, nn, endpoint=False)
    centres = [(0.5 * np.cos(t) + 0.1, 0.25 * np.sin(t), 0.15 * np.sin(2 * t)) for t in ang]
    ch = S.make_chain(500 + nn, 1991, centres, ["mono" if mono else "mixed"] * (nn + 1), mono, [6.0] * nn, nvis=0.5)
    cur = kf_of(ch["cur"])
    nbs = [pkg.newpoints_neighbour(kf_of(n["kf"]), n["cd"], n["cf"], n["nqs"], n["qi"], n["ncs"], n["ci"], n["F12"], n["ex"], n["ey"], n["median"]) for n in ch["nbs"]]
    nbk = [kf_of(n["kf"]) for n in ch["nbs"]]

    def chain():
        return pkg.create_new_map_points(cur, ch["qd"], ch["qf"], nbs, mono)

    def loop():
        flags = ch["qf"].copy()
        out = []
        for i, n in enumerate(ch["nbs"]):
            if not pkg.baseline_ok(ch["cur"]["view"], n["kf"]["view"], mono, n["median"]):
                out.append(None)
                continue
            _, mq = pkg.search_for_triangulation(ch["cur"]["kp"], ch["qd"], flags, n["kf"]["kp"], n["cd"], n["cf"], n["nqs"], n["qi"], n["ncs"], n["ci"], n["F12"],
                                                 n["ex"], n["ey"], n["kf"]["sf"], n["kf"]["sig2"], 50, False)
            idx1 = np.flatnonzero(mq >= 0)
            rows, _ = pkg.triangulate_new_points(cur, nbk[i], np.stack([idx1, mq[idx1]], axis=1))
            flags[idx1[rows["status"] >= 0]] &= 0xFE
            out.append((mq, idx1, rows))
        return out, flags
    c, (l, lf) = chain(), loop()
    assert (c["q_flags"] == lf).all()
    for i, e in enumerate(l):
        assert (e is None) == bool(c["skipped"][i])
        if e is not None:
            assert (c["match_q"][i] == e[0]).all() and c["points"][i][e[1]].tobytes() == e[2].tobytes()
    ct, lt = [], []
    for _ in range(WARM + CALLS):
        ct.append(timed(chain))
        lt.append(timed(loop))
    print("%d neighbours (%s rule), %d features, %d matches, %d new points, %d skipped | the chain, one call: %s | the host loop over the two entry points: %s"
          % (nn, "monocular" if mono else "stereo", len(ch["qf"]), c["nmatches"].sum(), c["nnew"].sum(), c["skipped"].sum(), stats(ct), stats(lt)), flush=True)
