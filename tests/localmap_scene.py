"""Scenes for the local map (orbt_*): one small map + frame per rule of Tracking::UpdateLocalMap, and what each must show on the
restatement's own result (tests/localmap_ref.py).  A scene is a dict: table, features (tests/covis_ref.py's builders), parent [K],
cov / children (lists of slots per keyframe), views, desc, frame_points, prev_kf, max_keyframes, nbest."""
import functools

import numpy as np

import covis_ref as R
import localmap_ref as LR

LDS_KEYFRAMES = 8192
SF = np.float32(1.2) ** np.arange(8, dtype=np.float32)


def make(kf_points, frame, bad_kf=(), bad_pts=(), P=None, parent=None, cov=None, children=None, prev_kf=(), max_keyframes=80, nbest=10, seed=1):
    """kf_points[k]: the point index (or -1) of every feature slot of keyframe k.  A point's observation by a keyframe is its first
    feature there.  Positions, views and descriptors are random but fixed by the seed; observations() is the list's length plus
    p % 3, so that it is not the length (a stereo observation counts 2)."""
    K = len(kf_points)
    if P is None:
        P = 1 + max([max(f, default=-1) for f in kf_points] + [max(frame, default=-1)])
    rng = np.random.default_rng(seed)
    kf = np.zeros(K, R.KEYFRAME_DTYPE)
    kf["id"] = np.arange(K)
    kf["bad"][list(bad_kf)] = 1
    pts = np.zeros(P, R.POINT_DTYPE)
    pts["pos"] = rng.normal(size=(P, 3)).astype(np.float32)
    pts["ref_kf"] = -1
    pts["bad"][list(bad_pts)] = 1
    rows, seen = [], set()
    for k, f in enumerate(kf_points):
        for idx, p in enumerate(f):
            if p >= 0 and (p, k) not in seen:
                seen.add((p, k))
                rows.append((p, k, idx, 0, 0))
    table = R.build_table(kf, pts, rows, SF)
    feats = []
    for f in kf_points:
        a = np.zeros(len(f), R.FEATURE_DTYPE)
        a["point"] = f
        feats.append(a)
    views = np.zeros(P, LR.VIEW_DTYPE)
    views["normal"] = rng.normal(size=(P, 3)).astype(np.float32)
    views["max_distance"] = rng.uniform(5, 9, P).astype(np.float32)
    views["min_distance"] = rng.uniform(0.1, 1, P).astype(np.float32)
    views["observations"] = np.diff(table["obs_off"]) + np.arange(P) % 3
    return {"table": table, "features": R.build_queries(np.arange(K), feats), "parent": np.array(parent if parent is not None else [-1] * K, np.int32).reshape(K),
            "cov": [list(c) for c in (cov if cov is not None else [[]] * K)], "children": [list(c) for c in (children if children is not None else [[]] * K)],
            "views": views, "desc": rng.integers(0, 256, (P, 32), dtype=np.uint8), "frame_points": np.array(frame, np.int32).reshape(len(frame)),
            "prev_kf": np.array(prev_kf, np.int32).reshape(len(prev_kf)), "max_keyframes": max_keyframes, "nbest": nbest}


def voted(S, extra=0, **kw):
    """S keyframes that own one point each, all named by the frame, and `extra` keyframes with one point of their own nobody names"""
    kw.setdefault("frame", list(range(S)))
    return [[k] for k in range(S + extra)], kw.pop("frame"), kw


def graph(K, parent=None, cov=None, children=None):
    pa, cv, ch = [-1] * K, [[] for _ in range(K)], [[] for _ in range(K)]
    for k, v in (parent or {}).items():
        pa[k] = v
    for k, v in (cov or {}).items():
        cv[k] = v
    for k, v in (children or {}).items():
        ch[k] = v
    return dict(parent=pa, cov=cv, children=ch)


def ext_scene(S, extra, bad_kf=(), **g):
    kp, fr, _ = voted(S, extra)
    return make(kp, fr, bad_kf=bad_kf, **graph(S + extra, **g))


# ---- the vote
def plain():
    return make([[0, 1, 2], [1, 2, 3], [3, 4], [5]], [0, 1, 2, -1])


def bad_frame_point():
    return make([[0, 1], [1, 2], [4, 4, 4]], [0, 4, 4, 4, 1], bad_pts=[4])


def point_twice_in_frame():
    return make([[0], [1, 2], [2]], [1, 1, 2])


def point_without_observations():
    return make([[0, 1], [1]], [1, 4, -1, 5], P=6)


def vote_tie():
    return make([[9], [0, 1], [0, 1], [2]], [0, 1, 2])


def bad_keyframe_has_most_votes():
    return make([[0], [0, 1, 2], [1, 2]], [0, 1, 2], bad_kf=[1])


def all_voted_bad():
    return make([[0, 1], [1], [5]], [0, 1], bad_kf=[0, 1], prev_kf=[2])


def empty_vote():
    return make([[0, 1], [2], [1, 3]], [-1, 4, -1], P=5, prev_kf=[2, 0])


def K_lds_plus_1():
    K = LDS_KEYFRAMES + 1
    kp = [[] for _ in range(K)]
    kp[5], kp[4000], kp[K - 1] = [0, 1], [1, 2, 3], [0, 1, 2, 4]
    return make(kp, [0, 1, 2, -1, 2], **graph(K, cov={5: [K - 2]}, parent={4000: 7}))


def _wave(N):
    kp = [[(3 * k + i) % N for i in range(7)] for k in range(40)]
    fr = [i if i % 9 else -1 for i in range(N)]
    return make(kp, fr, bad_pts=[4, 64], P=N)


def N_65():
    return _wave(65)


def N_130():
    return _wave(130)


# ---- the extension
def length_80_runs():
    return ext_scene(80, 3, cov={0: [80]}, children={0: [81]}, parent={0: 82})


def length_81_stops():
    return ext_scene(81, 1, cov={0: [81]})


def voted_100():
    return ext_scene(100, 1, cov={0: [100]}, parent={0: 100})


def neighbour_marked_falls_through():
    return ext_scene(2, 2, cov={0: [1, 2, 3]})


def bad_neighbour_skipped():
    return ext_scene(1, 2, bad_kf=[1], cov={0: [1, 2]})


def eleventh_neighbour_ignored():
    return ext_scene(11, 1, cov={0: list(range(1, 12))})


def children_70_last_free():
    return ext_scene(1, 70, bad_kf=range(1, 70), children={0: list(range(1, 71))})


def bad_child_skipped():
    return ext_scene(1, 2, bad_kf=[1], children={0: [1, 2]})


def parent_missing():
    return ext_scene(2, 2, cov={0: [2], 1: [3]})


def parent_marked():
    return ext_scene(2, 1, parent={0: 1}, cov={1: [2]})


def parent_bad_is_added():
    return ext_scene(1, 1, bad_kf=[1], parent={0: 1})


def parent_ends_the_loop():
    return ext_scene(2, 2, parent={0: 2}, cov={1: [3]})


def appended_not_visited():
    return ext_scene(1, 2, cov={0: [1], 1: [2]})


# ---- the points and the packing
def shared_point_first_occurrence():
    return make([[0, 1], [1, 2, 0], [7]], [0, 2])


def point_twice_in_one_keyframe():
    return make([[3, 3, 4, 3]], [4])


def bad_point_never_blocks():
    return make([[0, 1], [0, 2]], [1, 2], bad_pts=[0])


def null_slots():
    return make([[-1, 0, -1, -1, 1, -1], [-1, -1, 2]], [0, -1, 2])


def feature_counts_0_1_63_64_65_1025():
    counts = [0, 1, 63, 64, 65, 1025]
    kp = [[(7 * i + 3 * k) % 600 for i in range(c)] for k, c in enumerate(counts)]
    return make(kp, [-1, -1], P=600, prev_kf=[3, 0, 5, 1, 4, 2])


def m_0():
    return make([[-1, 0, -1], [0], []], [-1], bad_pts=[0], prev_kf=[1, 0, 2])


def m_257():
    return make([list(range(0, 200)), list(range(150, 300))], [0, 299, 5])


def frame_point_is_valid_0():
    return make([[0, 1, 2], [2, 3]], [1, -1, 3])


def random(seed=0, K=60, P=3000, N=500):
    rng = np.random.default_rng(100 + seed)
    kp = []
    for k in range(K):
        f = rng.integers(0, P, int(rng.integers(150, 400)))
        f[rng.random(len(f)) < 0.2] = -1
        kp.append([int(x) for x in f])
    parent = [-1] + [int(rng.integers(0, k)) for k in range(1, K)]
    children = [[c for c in range(K) if parent[c] == k] for k in range(K)]
    cov = [[int(x) for x in rng.permutation([c for c in range(K) if c != k])[:int(rng.integers(0, 25))]] for k in range(K)]
    near = kp[int(rng.integers(0, K))] + kp[int(rng.integers(0, K))]
    fr = [int(near[int(rng.integers(0, len(near)))]) if rng.random() < 0.7 else (int(rng.integers(0, P)) if rng.random() < 0.5 else -1) for _ in range(N)]
    return make(kp, fr, bad_kf=[int(x) for x in rng.choice(K, 6, replace=False)], bad_pts=[int(x) for x in rng.choice(P, 200, replace=False)], P=P,
                parent=parent, cov=cov, children=children, prev_kf=[3, 1], max_keyframes=int(rng.choice([80, 20])), seed=seed + 5)


SCENES = {f.__name__: f for f in (
    plain, bad_frame_point, point_twice_in_frame, point_without_observations, vote_tie, bad_keyframe_has_most_votes, all_voted_bad, empty_vote, K_lds_plus_1,
    N_65, N_130, length_80_runs, length_81_stops, voted_100, neighbour_marked_falls_through, bad_neighbour_skipped, eleventh_neighbour_ignored,
    children_70_last_free, bad_child_skipped, parent_missing, parent_marked, parent_bad_is_added, parent_ends_the_loop, appended_not_visited,
    shared_point_first_occurrence, point_twice_in_one_keyframe, bad_point_never_blocks, null_slots, feature_counts_0_1_63_64_65_1025, m_0, m_257,
    frame_point_is_valid_0, random)}
RANDOM_SEEDS_CPU = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def scene(name, seed=0):
    return SCENES[name](seed) if name == "random" else SCENES[name]()


@functools.lru_cache(maxsize=None)
def expected(name, seed=0):
    """computed once and shared; nobody writes into it"""
    return LR.update_local_map(scene(name, seed))


def assert_conditions(name):
    """what the scene is named for, on the restatement's result"""
    sc, o = scene(name), expected(name)
    i, kf, lp = o["info"], list(o["local_kf"]), list(o["local_pts"])
    K = len(sc["table"]["kf"])
    c = {
        "plain": lambda: i["ref_kf"] == 0 and i["ref_votes"] == 3 and kf == [0, 1] and lp == [0, 1, 2, 3] and list(o["holder"]) == [0, 1, 2, -1],
        "bad_frame_point": lambda: list(o["frame_points"]) == [0, -1, -1, -1, 1] and 2 not in o["counters"] and kf == [0, 1] and list(o["holder"]) == [0, -1, -1, -1, 1],
        "point_twice_in_frame": lambda: o["counters"][1] == 3 and i["ref_kf"] == 1 and i["ref_votes"] == 3,
        "point_without_observations": lambda: list(o["holder"]) == [1, -2, -1, -2] and list(o["ext_obs"]) == [0, 1, 0, 2],
        "vote_tie": lambda: o["counters"][1] == o["counters"][2] == 2 and i["ref_kf"] == 1,
        "bad_keyframe_has_most_votes": lambda: o["counters"][1] == 3 and i["ref_kf"] == 2 and i["ref_votes"] == 2 and kf == [0, 2],
        "all_voted_bad": lambda: i["empty_vote"] == 0 and kf == [] and i["ref_kf"] == -1 and i["n_voted"] == 0 and lp == [] and list(o["holder"]) == [-2, -2],
        "empty_vote": lambda: i["empty_vote"] == 1 and kf == [2, 0] and lp == [1, 3, 0] and i["ref_kf"] == -1 and list(o["holder"]) == [-1, -2, -1],
        "K_lds_plus_1": lambda: K == LDS_KEYFRAMES + 1 and kf == [5, 4000, K - 1, K - 2, 7] and i["ref_kf"] == K - 1 and i["extension_end"] == LR.END_PARENT,
        "N_65": lambda: len(sc["frame_points"]) == 65 and o["frame_points"][64] == -1 and sc["frame_points"][64] == 64,
        "N_130": lambda: len(sc["frame_points"]) == 130 and (o["holder"][128:] == -2).all() and (o["holder"][64:128] >= 0).sum() > 50,
        "length_80_runs": lambda: i["n_voted"] == 80 and kf[80:] == [80, 81, 82] and i["extension_end"] == LR.END_PARENT,
        "length_81_stops": lambda: i["n_voted"] == 81 and len(kf) == 81 and i["extension_end"] == LR.END_LENGTH,
        "voted_100": lambda: len(kf) == 100 and i["extension_end"] == LR.END_LENGTH,
        "neighbour_marked_falls_through": lambda: kf == [0, 1, 2] and i["extension_end"] == LR.END_RAN_OUT,
        "bad_neighbour_skipped": lambda: kf == [0, 2],
        "eleventh_neighbour_ignored": lambda: len(kf) == 11 and 11 not in kf,
        "children_70_last_free": lambda: kf == [0, 70],
        "bad_child_skipped": lambda: kf == [0, 2],
        "parent_missing": lambda: kf == [0, 1, 2, 3] and i["extension_end"] == LR.END_RAN_OUT,
        "parent_marked": lambda: kf == [0, 1, 2] and i["extension_end"] == LR.END_RAN_OUT,
        "parent_bad_is_added": lambda: kf == [0, 1] and sc["table"]["kf"]["bad"][1] == 1 and i["extension_end"] == LR.END_PARENT,
        "parent_ends_the_loop": lambda: kf == [0, 1, 2] and 3 not in kf and i["extension_end"] == LR.END_PARENT,
        "appended_not_visited": lambda: kf == [0, 1] and 2 not in kf and i["extension_end"] == LR.END_RAN_OUT,
        "shared_point_first_occurrence": lambda: kf == [0, 1] and lp == [0, 1, 2],
        "point_twice_in_one_keyframe": lambda: lp == [3, 4],
        "bad_point_never_blocks": lambda: lp == [1, 2] and kf == [0, 1],
        "null_slots": lambda: lp == [0, 1, 2],
        "feature_counts_0_1_63_64_65_1025": lambda: i["empty_vote"] == 1 and kf == [3, 0, 5, 1, 4, 2] and len(lp) == len(set(lp)) == 600,
        "m_0": lambda: len(kf) == 3 and lp == [] and len(o["pts"]) == 0,
        "m_257": lambda: len(lp) == 300 > 257 and lp == list(range(300)),
        "frame_point_is_valid_0": lambda: lp == [0, 1, 2, 3] and list(o["pts"]["valid"]) == [1, 0, 1, 0] and not o["mp_desc"][1].any() and o["mp_desc"][0].any()
        and o["pts"]["observations"][1] == sc["views"]["observations"][1] != 0 and o["pts"]["wx"][1] == 0 and list(o["holder"]) == [1, -1, 3],
        "random": lambda: len(kf) > i["n_voted"] > 5 and len(lp) > 1000 and (o["holder"] == -2).any() and (o["pts"]["valid"] == 0).any(),
    }[name]
    assert c(), (name, i, kf[:90], lp[:20], o["holder"][:10], o["ext_obs"][:10])
