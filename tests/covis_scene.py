"""Named scenes for the covisibility entry points.  A scene is built with the small builder below, which keeps the table consistent
(every observation (kf, idx) has feature idx of kf naming the point, and the other way round), and carries its own call arguments.
assert_conditions(name) checks on the restatement's own results (tests/covis_ref.py) that the scene shows what it is named for.

CONNECTION_CASES[name]() -> {"table", "queries", "th", "cap"}; CULLING_CASES[name]() -> {"table", "queries", "monocular", "th_obs"};
NORMAL_CASES[name]() -> {"table"}."""
import numpy as np

import covis_ref as R

F32 = np.float32
NLEVELS = 8
SF = np.array([1.2 ** l for l in range(NLEVELS)], F32)
LDS_KEYFRAMES = 8192     # the package's COVIS_LDS_KEYFRAMES (tests/test_covis_cpu.py checks they agree)
SORT_LDS = 1024          # the package's COVIS_SORT_LDS


class Builder:
    def __init__(self, K, seed=0):
        rng = np.random.default_rng(seed)
        self.K = K
        self.kf = np.zeros(K, R.KEYFRAME_DTYPE)
        self.kf["id"] = np.arange(K) + 1
        self.kf["Ow"] = rng.uniform(-5, 5, (K, 3)).astype(F32)
        self.kf["th_depth"] = 40.0
        self.pts, self.rows, self.feats = [], [], [[] for _ in range(K)]

    def point(self, obs, pos=(0.5, -0.25, 8.0), bad=0, ref="first", depth=10.0):
        """obs: (kf, octave, stereo) each; -> the point's index.  ref: "first" = the first observer, or a slot / -1"""
        p = len(self.pts)
        r = (obs[0][0] if obs else -1) if ref == "first" else ref
        self.pts.append((tuple(pos), r, bad, (0, 0, 0)))
        for k, octv, st in obs:
            self.rows.append((p, k, len(self.feats[k]), octv, st))
            self.feats[k].append((p, octv, depth))
        return p

    def feature(self, kf, point, octave=0, depth=10.0):
        """a feature without an observation of its own: a NULL slot (point -1) or a second feature naming a point"""
        self.feats[kf].append((point, octave, depth))

    def table(self):
        return R.build_table(self.kf, np.array(self.pts, R.POINT_DTYPE) if self.pts else np.zeros(0, R.POINT_DTYPE), self.rows, SF)

    def queries(self, slots):
        return R.build_queries(slots, [np.array(self.feats[s], R.FEATURE_DTYPE) if self.feats[s] else np.zeros(0, R.FEATURE_DTYPE) for s in slots])


def _share(b, a, k, n, extra=()):
    """n points seen by a and k (and extra), level 0, mono"""
    for _ in range(n):
        b.point([(a, 0, 0), (k, 0, 0)] + [(e, 0, 0) for e in extra])


def _conn(b, slots, th=15, cap=None):
    return {"table": b.table(), "queries": b.queries(slots), "th": th, "cap": b.K if cap is None else cap}


def conn_plain():
    b = Builder(6)
    for k, n in ((1, 20), (2, 17), (3, 15), (4, 14), (5, 3)):
        _share(b, 0, k, n)
    _share(b, 0, 1, 2, extra=(2, 3))
    return _conn(b, [0])


def conn_ties():
    b = Builder(6)
    for k, n in ((1, 16), (2, 16), (3, 16), (4, 20), (5, 15)):
        _share(b, 0, k, n)
    return _conn(b, [0])


def conn_below_threshold():
    b = Builder(5)
    for k, n in ((1, 7), (2, 9), (3, 9), (4, 2)):
        _share(b, 0, k, n)
    return _conn(b, [0])


def conn_empty():
    b = Builder(4)
    for _ in range(5):
        b.point([(0, 0, 0), (1, 0, 0)], bad=1)
    for _ in range(3):
        b.feature(0, -1)
    _share(b, 2, 3, 16)
    return _conn(b, [0, 2])


def conn_duplicate_point():
    b = Builder(3)
    for _ in range(8):
        p = b.point([(0, 0, 0), (1, 0, 0)])
        b.feature(0, p)
    _share(b, 0, 2, 15)
    return _conn(b, [0])


def conn_bad_points():
    b = Builder(3)
    _share(b, 0, 1, 14)
    for _ in range(6):
        b.point([(0, 0, 0), (1, 0, 0)], bad=1)
    _share(b, 0, 2, 15)
    return _conn(b, [0])


def conn_long_lists():
    K, s = 140, 70
    b = Builder(K)
    for n in (1, 63, 64, 65, 130):
        others = [k for k in range(K) if k != s][: n - 1] if n < 130 else [k for k in range(K) if k != s][5:134]
        b.point(sorted([(s, 0, 0)] + [(k, 0, 0) for k in others]))
    return _conn(b, [s], th=1)


def _random_conn(K, npts, Q, seed, th=3, cap=None):
    rng = np.random.default_rng(seed)
    b = Builder(K, seed)
    qs = sorted([0, K - 1] + [1 + int(x) for x in rng.permutation(K - 2)[:Q - 2]]) if Q > 1 else [K - 1]
    pool = sorted(set(qs) | set(int(x) for x in rng.integers(0, K, 12)) | {K - 1, K - 2, 0})
    for _ in range(npts):
        n = int(rng.integers(2, min(7, len(pool)) + 1))
        ks = sorted(int(x) for x in rng.choice(pool, n, replace=False))
        b.point([(k, int(rng.integers(0, NLEVELS)), int(rng.integers(0, 2))) for k in ks], bad=int(rng.random() < 0.05))
    for s in qs:
        b.feature(s, -1)
    return _conn(b, qs, th=th, cap=cap)


def conn_long_order():
    """a list longer than the in-LDS sort's limit, weights 1..3 so that ties run for hundreds of entries, and cap below n"""
    K = SORT_LDS + 476
    b = Builder(K)
    for k in range(1, SORT_LDS + 300):
        _share(b, 0, k, 1 + (k % 3))
    return _conn(b, [0], th=1, cap=100)


CONNECTION_CASES = {
    "plain": conn_plain, "ties": conn_ties, "below_threshold": conn_below_threshold, "empty": conn_empty, "duplicate_point": conn_duplicate_point,
    "bad_points": conn_bad_points, "long_lists": conn_long_lists, "long_order": conn_long_order,
    "K3": lambda: _random_conn(3, 60, 1, 1), "K64": lambda: _random_conn(64, 300, 1, 2), "K65": lambda: _random_conn(65, 300, 1, 3),
    "K_lds": lambda: _random_conn(LDS_KEYFRAMES, 300, 3, 4), "K_lds_plus_1": lambda: _random_conn(LDS_KEYFRAMES + 1, 300, 3, 5),
    "Q40": lambda: _random_conn(64, 400, 40, 6, th=1, cap=5),
}


# ---- culling.  A "redundant" point of keyframe a: seen by a and four others at a's level, so that it stays redundant for the others
# when one observer leaves; a "thin" one: seen by exactly four, so that it stops being redundant (nObs 3) when one leaves
def _cull(b, slots, monocular=1, th_obs=3):
    return {"table": b.table(), "queries": b.queries(slots), "monocular": monocular, "th_obs": th_obs}


A, B_, C_, D_, E_, F_, G_ = 1, 2, 3, 4, 5, 6, 7


def cull_chain():
    b = Builder(8)
    for _ in range(10):
        b.point([(A, 0, 0), (B_, 0, 0), (C_, 0, 0), (D_, 0, 0)])
    return _cull(b, [A, B_])


def cull_point_dies(b_stereo=0):
    b = Builder(8)
    for _ in range(10):
        b.point([(A, 0, 0), (C_, 0, 0), (D_, 0, 0), (E_, 0, 0), (F_, 0, 0)])
    for _ in range(9):
        b.point([(B_, 0, 0), (C_, 0, 0), (D_, 0, 0), (E_, 0, 0), (F_, 0, 0)])
    x = b.point([(A, 0, 0), (B_, 0, b_stereo), (C_, 0, 0)])
    sc = _cull(b, [A, B_])
    sc["x"] = x
    return sc


def cull_stereo_keeps_point():
    """point_dies with B's observation of x stereo: x keeps nObs 3 and lives, and B is not culled"""
    return cull_point_dies(b_stereo=1)


def cull_stereo_count():
    """Two stereo observations give nObs = 4 > 3 with only one other keyframe: A's first ten points pass the Observations() test and
    their lists are walked, but one other observer is fewer than three, so none is redundant; the same ten points with monocular
    observations (B's) have nObs 2 and are not walked.  No output of the call can tell the two apart - whenever three other
    observers exist, nObs > 3 holds anyway - so what is asserted by name is the restatement's trace; where the weight of a stereo
    observation changes an output is stereo_keeps_point."""
    b = Builder(8)
    for _ in range(10):
        b.point([(A, 0, 1), (C_, 0, 1)])
    for _ in range(10):
        b.point([(B_, 0, 0), (C_, 0, 0)])
    return _cull(b, [A, B_])


def cull_not_erase():
    b = Builder(8)
    b.kf["not_erase"][A] = 1
    for _ in range(10):
        b.point([(A, 0, 0), (B_, 0, 0), (C_, 0, 0), (D_, 0, 0)])
    return _cull(b, [A, B_])


def cull_id0():
    b = Builder(8)
    b.kf["id"][A] = 0
    for _ in range(10):
        b.point([(A, 0, 0), (B_, 0, 0), (C_, 0, 0), (D_, 0, 0)])
    return _cull(b, [A, B_])


def cull_stereo_far(monocular=0):
    b = Builder(8)
    for _ in range(10):
        b.point([(A, 0, 1), (C_, 0, 1), (D_, 0, 1), (E_, 0, 1)], depth=10.0)
    for _ in range(5):
        b.point([(A, 0, 0), (C_, 0, 0)], depth=50.0)
    for _ in range(3):
        b.point([(A, 0, 0), (C_, 0, 0)], depth=-1.0)
    b.point([(A, 0, 1), (C_, 0, 1)], depth=40.0)   # == th_depth: kept (the test is `>`); not redundant
    return _cull(b, [A], monocular=monocular)


def cull_level_edge():
    b = Builder(8)
    for _ in range(10):
        b.point([(A, 2, 0), (C_, 3, 0), (D_, 3, 0), (E_, 4, 0)])
    for _ in range(10):
        b.point([(B_, 2, 0), (C_, 3, 0), (D_, 3, 0), (E_, 3, 0)])
    return _cull(b, [A, B_])


def cull_ninety():
    b = Builder(8)
    for _ in range(9):
        b.point([(A, 0, 0), (C_, 0, 0), (D_, 0, 0), (E_, 0, 0)])
    b.point([(A, 0, 0), (C_, 0, 0)])
    for _ in range(10):
        b.point([(B_, 0, 0), (C_, 0, 0), (D_, 0, 0), (E_, 0, 0)])
    return _cull(b, [A, B_])


def cull_none_culled():
    b = Builder(8)
    for a in (A, B_, C_):
        for _ in range(10):
            b.point([(a, 0, 0), (D_, 0, 0), (E_, 0, 0)])
    return _cull(b, [A, B_, C_])


def cull_all_culled():
    b = Builder(8)
    for _ in range(12):
        b.point([(k, 0, 0) for k in range(8)])
    return _cull(b, [A, B_, C_, D_])


def cull_random(seed=11, K=40, Q=30, npts=300, monocular=0):
    rng = np.random.default_rng(seed)
    b = Builder(K, seed)
    b.kf["not_erase"][rng.integers(0, K, K // 4)] = 1
    b.kf["id"][0] = 0
    for _ in range(npts):
        n = int(rng.integers(3, 8))
        ks = sorted(int(x) for x in rng.choice(K // 2 if rng.random() < 0.7 else K, n, replace=False))
        lvl = int(rng.integers(0, NLEVELS - 2))
        b.point([(k, lvl + int(rng.integers(0, 3)), int(rng.random() < 0.3)) for k in ks], bad=int(rng.random() < 0.03),
                depth=float(rng.choice([5.0, 20.0, 45.0, -1.0], p=[0.5, 0.3, 0.15, 0.05])))
    b.point([(k, 1, 0) for k in range(K) if k % 5 != 4][:30] if K < 130 else [(k, 1, 0) for k in range(130)])
    qs = [int(x) for x in rng.permutation(K)[:Q]]
    for s in qs:
        b.feature(s, -1)
    return _cull(b, qs, monocular=monocular)


CULLING_CASES = {
    "chain": cull_chain, "point_dies": cull_point_dies, "not_erase": cull_not_erase, "id0": cull_id0, "stereo_far": cull_stereo_far,
    "stereo_far_monocular": lambda: cull_stereo_far(1), "level_edge": cull_level_edge, "stereo_count": cull_stereo_count, "stereo_keeps_point": cull_stereo_keeps_point, "ninety": cull_ninety,
    "none_culled": cull_none_culled, "all_culled": cull_all_culled, "random": cull_random,
    "random_long_lists": lambda: cull_random(12, K=140, Q=100, npts=200, monocular=1),
}


# ---- normals
def normals_lists():
    K = 200
    b = Builder(K, 3)
    rng = np.random.default_rng(3)
    for n in (1, 2, 64, 65, 200):
        ks = sorted(int(x) for x in rng.choice(K, n, replace=False))
        b.point([(k, int(rng.integers(0, NLEVELS)), 0) for k in ks], pos=tuple(rng.uniform(-3, 3, 3) + (0, 0, 9)), ref=ks[n // 2])
    return {"table": b.table()}


def normals_status():
    b = Builder(6, 4)
    ok = b.point([(0, 1, 0), (2, 3, 0)], ref=2)
    bad = b.point([(0, 1, 0), (2, 3, 0)], bad=1)
    empty = b.point([], ref=-1)
    empty_ref = b.point([], ref=3)
    noref = b.point([(0, 1, 0), (2, 3, 0)], ref=-1)
    absent = b.point([(0, 1, 0), (2, 3, 0)], ref=1)
    return {"table": b.table(), "want": {ok: R.NORMAL_OK, bad: R.NORMAL_BAD, empty: R.NORMAL_NO_OBSERVATION, empty_ref: R.NORMAL_NO_OBSERVATION,
                                         noref: R.NORMAL_NO_REFERENCE, absent: R.NORMAL_NO_REFERENCE}}


def normals_near_far():
    K = 12
    b = Builder(K, 5)
    rng = np.random.default_rng(5)
    for i in range(300):
        ks = sorted(int(x) for x in rng.choice(K, int(rng.integers(1, 9)), replace=False))
        c = b.kf["Ow"][ks[0]].astype(np.float64)
        scale = [1e-3, 0.05, 3.0, 200.0, 1e4, 1e7][i % 6]
        b.point([(k, int(rng.integers(0, NLEVELS)), 0) for k in ks], pos=tuple(c + rng.normal(size=3) * scale), ref=ks[int(rng.integers(0, len(ks)))])
    return {"table": b.table()}


NORMAL_CASES = {"lists": normals_lists, "status": normals_status, "near_far": normals_near_far}


def assert_conditions(kind, name):
    if kind == "connections":
        sc = CONNECTION_CASES[name]()
        res = R.update_connections(sc["table"], sc["queries"], sc["th"])
        ids, ws, cnt = res[0]
        if name == "plain":
            assert ids == [1, 2, 3] and ws == [22, 19, 17] and cnt[4] == 14 and cnt[5] == 3
        elif name == "ties":
            assert ids == [4, 3, 2, 1, 5] and ws == [20, 16, 16, 16, 15]
        elif name == "below_threshold":
            assert ids == [2] and ws == [9] and cnt[3] == 9 and max(cnt.values()) < sc["th"]
        elif name == "empty":
            assert ids == [] and cnt == {} and res[1][0] == [3]
        elif name == "duplicate_point":
            assert ids == [1, 2] and ws == [16, 15]
        elif name == "bad_points":
            assert ids == [2] and ws == [15] and cnt[1] == 14
        elif name == "long_lists":
            lens = sorted(np.diff(sc["table"]["obs_off"]).tolist())
            assert lens == [1, 63, 64, 65, 130] and len(ids) == 134
        elif name == "long_order":
            assert len(ids) > SORT_LDS and sc["cap"] < len(ids) and len(set(ws)) == 3
        elif name in ("K_lds", "K_lds_plus_1", "K3", "K64", "K65"):
            assert len(sc["table"]["kf"]) == {"K_lds": LDS_KEYFRAMES, "K_lds_plus_1": LDS_KEYFRAMES + 1, "K3": 3, "K64": 64, "K65": 65}[name]
            assert any(len(r[0]) > 0 for r in res)
            if name != "K3":
                assert any(len(sc["table"]["kf"]) - 1 in r[2] or len(sc["table"]["kf"]) - 2 in r[2] for r in res)   # the last slots are counted
        elif name == "Q40":
            assert len(res) == 40 and any(len(r[0]) > sc["cap"] for r in res)
    elif kind == "culling":
        sc = CULLING_CASES[name]()
        nm, nr, v, pb, trace = R.keyframe_culling(sc["table"], sc["queries"], sc["monocular"], sc["th_obs"])
        alone = [R.keyframe_culling(sc["table"], R.build_queries([s], [sc["queries"]["feat"][sc["queries"]["feat_off"][q]:sc["queries"]["feat_off"][q + 1]]]),
                                    sc["monocular"], sc["th_obs"]) for q, s in enumerate(sc["queries"]["query_kf"])] if len(v) <= 4 else None
        if name == "chain":
            assert list(v) == [1, 0] and alone[1][2][0] == 1 and nm[1] == alone[1][0][0] and nr[1] == 0
        elif name == "point_dies":
            assert list(v) == [1, 1] and alone[1][2][0] == 0 and alone[1][0][0] == 10 and nm[1] == 9 and pb[sc["x"]] == 1
        elif name == "stereo_keeps_point":
            assert list(v) == [1, 0] and nm[1] == 10 and pb[sc["x"]] == 0
        elif name == "stereo_count":
            assert list(v) == [0, 0] and list(nm) == [10, 10] and list(nr) == [0, 0]
            assert trace[0]["nobs_walked"] == [4] * 10 and trace[1]["nobs_walked"] == []
        elif name == "not_erase":
            assert list(v) == [2, 1] and not pb.any()
        elif name == "id0":
            assert list(v) == [0, 1] and nm[0] == 0 and nr[0] == 0
        elif name == "stereo_far":
            assert list(v) == [1] and nm[0] == 11 and nr[0] == 10 and trace[0]["skipped_far"] == 8
        elif name == "stereo_far_monocular":
            assert list(v) == [0] and nm[0] == 19 and nr[0] == 10
        elif name == "level_edge":
            assert list(v) == [0, 1] and nr[0] == 0 and nr[1] == 10 and trace[0]["level_rejects"] == 10
        elif name == "ninety":
            assert list(v) == [0, 1] and (nm[0], nr[0]) == (10, 9) and (nm[1], nr[1]) == (10, 10)
        elif name == "none_culled":
            assert not v.any() and nm.all()
        elif name == "all_culled":
            assert (v == 1).all()
        else:
            assert (v == 1).any() and (v == 2).any() and (v == 0).any() and pb.any()
    else:
        sc = NORMAL_CASES[name]()
        out = R.update_normal_and_depth(sc["table"])
        if name == "lists":
            assert sorted(np.diff(sc["table"]["obs_off"]).tolist()) == [1, 2, 64, 65, 200] and (out["status"] == 0).all()
            assert (np.abs(np.linalg.norm(out["normal"], axis=1)) <= 1.0 + 1e-5).all() and (out["max_distance"] > out["min_distance"]).all()
        elif name == "status":
            for p, s in sc["want"].items():
                assert out["status"][p] == s
            z = out[out["status"] != 0]
            assert not z["normal"].any() and not z["max_distance"].any() and not z["min_distance"].any()
        else:
            ok = out[out["status"] == 0]
            assert len(ok) == len(out) and np.isfinite(ok["normal"]).all() and ok["max_distance"].min() < 0.1 and ok["max_distance"].max() > 1e6


def expected_connections(sc):
    """the restatement's result in the entry point's layout: ids, weights [Q, cap] (-1 beyond min(n, cap)), n [Q], counters [Q, K]"""
    res = R.update_connections(sc["table"], sc["queries"], sc["th"])
    Q, K, cap = len(res), len(sc["table"]["kf"]), sc["cap"]
    ids, ws, n, cnt = np.full((Q, cap), -1, np.int32), np.full((Q, cap), -1, np.int32), np.zeros(Q, np.int32), np.zeros((Q, K), np.int32)
    for q, (i, w, c) in enumerate(res):
        m = min(len(i), cap)
        ids[q, :m], ws[q, :m], n[q] = i[:m], w[:m], len(i)
        for k, v in c.items():
            cnt[q, k] = v
    return ids, ws, n, cnt


def expected_culling(sc):
    return R.keyframe_culling(sc["table"], sc["queries"], sc["monocular"], sc["th_obs"])[:4]
