"""Seeded scenes for the loop map correction (tests/mapcorrect_ref.py is the restatement).  The smallest shapes that still cross every
boundary: more points and more features than one workgroup (256), queries on non-contiguous slots, the current keyframe not last.

LOOP_SCENES (orbr_correct_loop / correct_loop_map):
  q1          Q = 1: the current keyframe alone, s != 1
  scaled      K = 12, Q = 5 on slots 1 3 4 8 10, cur = 8 (position 3), s = 1.3
  unit_scale  the same map, s == 1
Special points of the K = 12 map (SPECIAL): `third` is owned by the third query and observed by the two earlier queries (whose features
do not name it), its owner, a later query and a keyframe that is not a query; `twice` is named twice by one keyframe; `bad` is bad and
named; `empty` has an empty list and is named; `noref` has ref_kf -1; `strayref` has a ref_kf outside its list; `unseen` is named by no
query.
SPREAD_SCENES (orbr_spread_global_ba / spread_global_ba):
  tree        K = 14, two origins (0, 9); 1 -> 3 -> 4 -> 5 outside the global BA under 1 inside (three levels), 8 inside under 5; 6 and 7
              siblings outside under 2; 11 outside under 10; 12 (inside) and 13 (outside) in nobody's child list with a parent pointer,
              both referred to by points
  exact       the same tree with poses of signed permutations and small integers and TcwGBA == Tcw: every product is exact"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import covis_ref as CR          # noqa: E402
import mapcorrect_ref as MR     # noqa: E402

F32, F64 = np.float32, np.float64
QUERY_SLOTS, CUR = [1, 3, 4, 8, 10], 8
SPECIAL = {"third": 0, "twice": 1, "bad": 2, "empty": 3, "noref": 4, "strayref": 5, "unseen": 6}
NLEVELS = 8


def rotation(rng, angle):
    a = rng.normal(size=3)
    a = a / np.linalg.norm(a) * angle
    th = np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]]) / max(th, 1e-12)
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def pose(rng, angle=0.4, spread=2.0):
    T = np.eye(4, dtype=F32)
    T[:3, :3] = rotation(rng, angle * rng.uniform(0.2, 1.0)).astype(F32)
    T[:3, 3] = rng.uniform(-spread, spread, 3).astype(F32)
    return T


def _loop_map(rng, K, query_slots, P, nfeat):
    """-> table, queries, Tcw [K]: every keyframe observes a random subset of the points; a query's features name what it observes"""
    Tcw = [pose(rng) for _ in range(K)]
    kf = np.zeros(K, CR.KEYFRAME_DTYPE)
    for k in range(K):
        kf["id"][k], kf["Ow"][k], kf["th_depth"][k] = k + 1, MR.set_pose(Tcw[k])[0], 40.0
    pts = np.zeros(P, CR.POINT_DTYPE)
    pts["pos"] = rng.uniform(-4, 4, (P, 3)).astype(F32) + np.array([0, 0, 8], F32)
    feats = [np.full(nfeat, -1, np.int64) for _ in range(K)]
    octs = [rng.integers(0, NLEVELS, nfeat) for _ in range(K)]      # mvKeysUn[i].octave: an observation's octave is its feature's
    used = [0] * K
    rows, observers = [], [[] for _ in range(P)]

    def observe(p, k, name=True):
        i = used[k]
        used[k] += 1 + int(rng.integers(0, 2))      # leaves -1 slots behind
        assert i < nfeat
        if name:
            feats[k][i] = p
        rows.append((p, k, i, int(octs[k][i]), int(rng.integers(0, 2))))
        observers[p].append(k)
        return i

    sp = SPECIAL
    first_free = len(sp) if K > 1 else 0
    if K > 1:
        for k in (0, 4, 8):
            observe(sp["third"], k)
        for k in (1, 3):
            observe(sp["third"], k, name=False)
        for k in (3, 10):
            observe(sp["twice"], k)
        feats[3][nfeat - 1] = sp["twice"]      # named a second time by slot 3
        for k in (1, 4, 5):
            observe(sp["bad"], k)
        pts["bad"][sp["bad"]] = 1
        feats[4][nfeat - 2] = sp["empty"]      # named, but its list is empty
        for k in (3, 8, 9):
            observe(sp["noref"], k)
        for k in (1, 10):
            observe(sp["strayref"], k)
        for k in (0, 2, 5):
            observe(sp["unseen"], k)
    for p in range(first_free, P):
        n = int(rng.integers(1, min(K, 5) + 1))
        for k in sorted(rng.choice(K, n, replace=False)):
            observe(p, int(k))
    assert max(used) <= nfeat - 2
    for p in range(P):
        pts["ref_kf"][p] = observers[p][int(rng.integers(0, len(observers[p])))] if observers[p] else -1
    if K > 1:
        pts["ref_kf"][sp["third"]] = 4
        pts["ref_kf"][sp["noref"]] = -1
        pts["ref_kf"][sp["strayref"]] = 7
        pts["ref_kf"][sp["empty"]] = 4
    table = CR.build_table(kf, pts, rows, [F32(1.2) ** i for i in range(NLEVELS)])
    fq = []
    for k in query_slots:
        f = np.zeros(nfeat, CR.FEATURE_DTYPE)
        f["point"], f["octave"], f["depth"] = feats[k], octs[k], rng.uniform(1, 30, nfeat)
        fq.append(f)
    return table, CR.build_queries(query_slots, fq), np.stack(Tcw)


def _scw(rng, Tcur, s):
    """mg2oScw: the current keyframe's pose moved a little, with scale s"""
    T = Tcur.astype(F64).copy()
    T[:3, :3] = rotation(rng, 0.15) @ T[:3, :3]
    T[:3, 3] += rng.uniform(-0.5, 0.5, 3)
    S = MR.sim3_of_pose(T)
    return MR.record_of_sim3((S[0], S[1], np.array([s], F64)))


def _loop_scene(name):
    if name == "q1":
        rng = np.random.default_rng(361)
        table, queries, Tcw = _loop_map(rng, 1, [0], 300, 700)
        return {"table": table, "queries": queries, "cur": 0, "Tiw": Tcw[[0]], "Tcw": Tcw, "Scw": _scw(rng, Tcw[0], 0.8)}
    rng = np.random.default_rng(362)
    table, queries, Tcw = _loop_map(rng, 12, QUERY_SLOTS, 300, 200)
    return {"table": table, "queries": queries, "cur": CUR, "Tiw": Tcw[QUERY_SLOTS], "Tcw": Tcw, "Scw": _scw(rng, Tcw[CUR], 1.3 if name == "scaled" else 1.0)}


TREE_CHILDREN = [[1, 2], [3], [6, 7], [4], [5], [8], [], [], [], [10], [11], [], [], []]
TREE_IN_GBA = [1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 1, 0, 1, 0]
TREE_PARENT = [-1, 0, 0, 1, 3, 4, 2, 2, 5, -1, 9, 10, 2, 6]      # 12 and 13 keep a parent whose child set has forgotten them
TREE_ORIGINS = [0, 9]


def _exact_pose(rng):
    T = np.eye(4, dtype=F32)
    perm = rng.permutation(3)
    for r in range(3):
        T[r, :3] = 0
        T[r, perm[r]] = rng.choice([-1.0, 1.0])
    T[:3, 3] = rng.integers(-8, 9, 3)
    return T


def _spread_scene(name):
    rng = np.random.default_rng(363)
    K, P = len(TREE_CHILDREN), 300
    exact = name == "exact"
    Tcw = np.stack([_exact_pose(rng) if exact else pose(rng) for _ in range(K)])
    gba = np.zeros((K, 4, 4), F32)
    for k in range(K):
        if exact:
            gba[k] = Tcw[k]
        elif TREE_IN_GBA[k]:
            gba[k] = Tcw[k]
            gba[k][:3, :3] = (rotation(rng, 0.05) @ Tcw[k][:3, :3].astype(F64)).astype(F32)
            gba[k][:3, 3] += rng.uniform(-0.2, 0.2, 3).astype(F32)
    ref = rng.integers(0, K, P).astype(np.int32)
    ref[:K] = np.arange(K)      # every keyframe is some point's reference
    ref[K:K + 3] = -1
    in_gba = (rng.uniform(size=P) < 0.4).astype(np.uint8)
    in_gba[:K + 3] = 0
    bad = (rng.uniform(size=P) < 0.06).astype(np.uint8)
    bad[:K + 3] = 0
    bad[K + 3], in_gba[K + 3] = 1, 1      # bad wins over mPosGBA
    return {"Tcw": Tcw, "TcwGBA": gba, "kf_in_gba": np.array(TREE_IN_GBA, np.uint8), "children": TREE_CHILDREN, "parent": np.array(TREE_PARENT, np.int32),
            "origins": np.array(TREE_ORIGINS, np.int32), "pos": (rng.uniform(-4, 4, (P, 3)) + [0, 0, 8]).astype(F32), "posGBA": rng.uniform(-4, 4, (P, 3)).astype(F32),
            "pt_in_gba": in_gba, "ref_kf": ref, "bad": bad}


LOOP_SCENES = ("q1", "scaled", "unit_scale")
SPREAD_SCENES = ("tree", "exact")
_cache = {}


def loop_scene(name):
    if ("loop", name) not in _cache:
        _cache[("loop", name)] = _loop_scene(name)
    return _cache[("loop", name)]


def spread_scene(name):
    if ("spread", name) not in _cache:
        _cache[("spread", name)] = _spread_scene(name)
    return _cache[("spread", name)]


def loop_poses(name):
    """GetPose() of every keyframe of a loop scene [K, 4, 4]; the table's Ow are their camera centres"""
    return loop_scene(name)["Tcw"]


def child_lists(sc):
    off = np.zeros(len(sc["children"]) + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in sc["children"]])
    return off, np.array([c for cs in sc["children"] for c in sorted(cs)], np.int32).reshape(-1)


def loop_expected(name, mutation=None):
    """computed once per (scene, mutation); callers must not write into it"""
    key = ("loop_expected", name, mutation)
    if key not in _cache:
        sc = loop_scene(name)
        _cache[key] = MR.correct_loop(sc["table"], sc["queries"], sc["cur"], sc["Tiw"], sc["Scw"], mutation)
    return _cache[key]


def spread_expected(name, mutation=None):
    key = ("spread_expected", name, mutation)
    if key not in _cache:
        _cache[key] = MR.spread_global_ba(spread_scene(name), mutation)
    return _cache[key]
