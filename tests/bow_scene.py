"""Synthetic DBoW2 vocabularies (no vocabulary file ships with the reference) and feature sets for the
BoW tests: a k-ary tree whose children are bit-flipped copies of their parent, in file (= node id) order
with parent < child, some leaves above the last level and some stopped words (weight 0).

Further down: the generators and the fixed cases of tests/test_bow_cpu.py and tests/test_bow_gpu.py - a vocabulary with
1 .. 33 children per node and planted ties (make_wide_vocabulary), a deep pruned one, vocabulary nodes crowded with up to
4096 candidates (crowded_nodes), best / runner-up pairs planted at chosen list positions and distances (planted_pairs),
one pair per node with chosen angles (singleton_nodes), and the SearchForTriangulation comparisons one float step to
either side (tri_edge_cases).  Each case is built once per process from fixed seeds and never modified."""
import numpy as np


def make_vocabulary(rng, k=10, L=3, early_leaf=0.05, stopped=0.05):
    parent, is_leaf, desc, weight, level = [0], [0], [np.zeros(32, np.uint8)], [0.0], [0]
    frontier = [0]
    for lv in range(1, L + 1):
        nxt = []
        for p in frontier:
            for _ in range(k):
                nid = len(parent)
                if p == 0:
                    d = rng.integers(0, 256, 32, dtype=np.uint8)
                else:
                    flips = np.zeros(256, np.uint8)
                    flips[rng.choice(256, max(4, 128 >> lv), replace=False)] = 1
                    d = desc[p] ^ np.packbits(flips)
                leaf = lv == L or (lv >= 2 and rng.random() < early_leaf)
                parent.append(p); desc.append(d); level.append(lv)
                is_leaf.append(1 if leaf else 0)
                weight.append(0.0 if (not leaf or rng.random() < stopped) else float(rng.uniform(0.1, 9.0)))
                if not leaf:
                    nxt.append(nid)
        frontier = nxt
    return dict(k=k, L=L, parent=np.array(parent, np.int32), is_leaf=np.array(is_leaf, np.uint8),
                desc=np.stack(desc), weight=np.array(weight, np.float64), level=np.array(level, np.int32))


def write_text(voc, path, scoring=0, weighting=0):
    """TemplatedVocabulary::saveToTextFile format (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1441-1470)."""
    with open(path, "w") as f:
        f.write("%d %d  %d %d\n" % (voc["k"], voc["L"], scoring, weighting))
        for i in range(1, len(voc["parent"])):
            f.write("%d %d %s %r\n" % (voc["parent"][i], voc["is_leaf"][i], " ".join(str(int(b)) for b in voc["desc"][i]),
                                       float(voc["weight"][i])))


def features_near_words(rng, voc, n, noise_bits=6):
    leaves = np.flatnonzero(voc["is_leaf"] == 1)
    pick = rng.choice(leaves, n)
    d = voc["desc"][pick].copy()
    for i in range(n):
        flips = np.zeros(256, np.uint8)
        flips[rng.choice(256, rng.integers(0, noise_bits + 1), replace=False)] = 1
        d[i] ^= np.packbits(flips)
    far = rng.random(n) < 0.1
    d[far] = rng.integers(0, 256, (int(far.sum()), 32), dtype=np.uint8)
    return d


def intersect(fv_q, fv_c):
    """The merge loop of src/ORBmatcher.cc:176-248: common nodes in increasing id -> CSR lists."""
    nqs, qit, ncs, cit = [0], [], [0], []
    for node in sorted(set(fv_q) & set(fv_c)):
        qit += fv_q[node]; cit += fv_c[node]
        nqs.append(len(qit)); ncs.append(len(cit))
    return np.array(nqs, np.int32), np.array(qit, np.int32), np.array(ncs, np.int32), np.array(cit, np.int32)


# ---- shapes under which every branch of the BoW kernels runs (tests/test_bow_cpu.py, tests/test_bow_gpu.py) ----------
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"),
                     ("class_id", "<i4")])
WIDE_COUNTS = (1, 15, 16, 17, 20, 32, 33)


def _bits(rng, n, lo, hi):
    """[n, 32] masks with between lo and hi (inclusive) random bits set"""
    m = np.zeros((n, 256), np.uint8)
    for i in range(n):
        m[i, rng.choice(256, int(rng.integers(lo, hi + 1)), replace=False)] = 1
    return np.packbits(m, axis=1)


def _flip(rng, d, nbits, keep=None):
    """d with nbits random bits flipped, none of them where the mask `keep` is set"""
    free = np.arange(256) if keep is None else np.flatnonzero(np.unpackbits(keep) == 0)
    m = np.zeros(256, np.uint8)
    m[rng.choice(free, nbits, replace=False)] = 1
    return d ^ np.packbits(m)


def make_wide_vocabulary(rng):
    """An explicit tree (k = 20 in the header, L = 4) whose nodes have 1, 15, 16, 17, 20, 32 and 33 children: the root
    has 20; its first seven children have WIDE_COUNTS children each, the other thirteen are words at depth 1 (the
    last one childless but NOT flagged as a word: Node()'s word 0, weight 0); wide nodes again at depths 2 and 3; a
    chain of single-child nodes root-child 0 -> B -> C -> D.  Planted sibling ties, each with a probe feature that is
    equally far from both and nearer to them than to every other sibling:
        children 2 and 18 of the 20-child node identical (the first, child 2, must win across the 16-stride)
        children 0 and 16 of the 17-child node identical (child 0 must win)
        child 17 of the 32-child node strictly best, children 1, 16 and 18 one bit behind
        the 33rd child (position 32, the third step of the stride) of the 33-child node strictly best, children 0 and
        16 one bit behind
    voc["probes"]: (name, feature, node the descent must choose at depth 2)."""
    parent, desc, level = [0], [np.zeros(32, np.uint8)], [0]

    def add(p, d):
        parent.append(p); desc.append(np.asarray(d, np.uint8)); level.append(level[p] + 1)
        return len(parent) - 1

    def grow(p, n, nbits):
        return [add(p, _flip(rng, desc[p], nbits)) for _ in range(n)]

    A = [add(0, rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(20)]
    B = {n: grow(A[i], n, 24) for i, n in enumerate(WIDE_COUNTS)}
    probes = []

    def plant(name, kids, best, behind, same=None):
        flips = _flip(rng, np.zeros(32, np.uint8), 2)
        probe = desc[kids[best]] ^ flips
        if same is not None:
            desc[kids[same]] = desc[kids[best]].copy()
        for c in behind:                                   # one more differing bit than the best child
            desc[kids[c]] = _flip(rng, desc[kids[best]], 1, keep=flips)
        probes.append((name, probe, kids[best]))

    plant("tie_2_18", B[20], 2, (), same=18)
    plant("tie_0_16", B[17], 0, (), same=16)
    plant("best_17", B[32], 17, (1, 16, 18))
    plant("best_33rd", B[33], 32, (0, 16))
    grow(B[15][3], 17, 12)
    c33 = grow(B[15][7], 33, 12)
    grow(B[16][15], 20, 12)
    grow(B[32][20], 32, 12)
    grow(B[33][31], 16, 12)
    grow(c33[32], 15, 6)
    grow(grow(B[1][0], 1, 12)[0], 1, 6)                    # the chain A[0] -> B -> C -> D
    n = len(parent)
    parent = np.array(parent, np.int32)
    childless = np.bincount(parent[1:], minlength=n) == 0
    childless[0] = False
    is_leaf = childless.astype(np.uint8)
    is_leaf[A[19]] = 0
    weight = np.where(is_leaf == 1, rng.uniform(0.1, 9.0, n), 0.0)
    weight[rng.random(n) < 0.05] = 0.0
    return dict(k=20, L=4, parent=parent, is_leaf=is_leaf, desc=np.stack(desc), weight=weight.astype(np.float64),
                level=np.array(level, np.int32), probes=probes)


def _scene(rng, qd, cd, nqs, ncs, extra_q=0, extra_c=0):
    """Place the list-ordered descriptors at permuted feature indices (so that cit[p] != p); extra_* features belong
    to no node.  -> dict(qd, cd, nqs, qit, ncs, cit) + the permutations."""
    nq, nc = len(qd) + extra_q, len(cd) + extra_c
    pq, pc = rng.permutation(nq), rng.permutation(nc)
    Q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    Cc = rng.integers(0, 256, (nc, 32), dtype=np.uint8)
    qit, cit = pq[:len(qd)].astype(np.int32), pc[:len(cd)].astype(np.int32)
    Q[qit] = qd
    Cc[cit] = cd
    return dict(qd=Q, cd=Cc, nqs=np.asarray(nqs, np.int32), qit=qit, ncs=np.asarray(ncs, np.int32), cit=cit)


def crowded_nodes(sizes_q, sizes_c, seed, twins=0.0):
    """One cluster of descriptors per node: sizes_c[j] candidates within 60 bits of the node's centre, sizes_q[j]
    queries that are copies of random candidates with up to 12 bits of noise (several queries share a source: they
    contend for one candidate).  twins: the share of a node's candidates that are exact copies of another one (equal
    distances to every query).  -> the four CSR arrays nqs, qit, ncs, cit and qd, qa, qv, cd, ca, cv, plus q_group /
    c_group: the descriptor a feature was copied from (-1: none)."""
    r = np.random.default_rng(seed)
    qd, cd, nqs, ncs, qg, cg, g0 = [], [], [0], [0], [], [], 0
    for a, b in zip(sizes_q, sizes_c):
        centre = r.integers(0, 256, 32, dtype=np.uint8)
        m = max(1, int(round(b * (1.0 - twins)))) if b else 0
        pool = centre ^ _bits(r, m, 0, 60)
        grp = np.concatenate([np.arange(m), r.integers(0, m, b - m)]).astype(np.int64) if b else np.zeros(0, np.int64)
        r.shuffle(grp)
        src = r.integers(0, b, a) if b else np.zeros(a, np.int64)
        q = (pool[grp[src]] if b else np.tile(centre, (a, 1))) ^ _bits(r, a, 0, 12)
        qd.append(q); cd.append(pool[grp].reshape(-1, 32))
        qg.append(g0 + grp[src] if b else np.full(a, -1)); cg.append(g0 + grp)
        g0 += m
        nqs.append(nqs[-1] + a); ncs.append(ncs[-1] + b)
    s = _scene(r, np.concatenate(qd), np.concatenate(cd), nqs, ncs)
    nq, nc = len(s["qd"]), len(s["cd"])
    s["q_group"] = np.full(nq, -1, np.int64); s["q_group"][s["qit"]] = np.concatenate(qg)
    s["c_group"] = np.full(nc, -1, np.int64); s["c_group"][s["cit"]] = np.concatenate(cg)
    s["qa"] = r.uniform(0, 360, nq).astype(np.float32)
    s["ca"] = ((s["qa"].mean() + r.normal(0, 40, nc)) % 360).astype(np.float32)
    s["qv"] = (r.random(nq) > 0.1).astype(np.uint8)
    s["cv"] = (r.random(nc) > 0.15).astype(np.uint8)
    return s


def planted_pairs(pairs, nc, seed, invalid=()):
    """One node of nc candidates and one query per entry of pairs = [(p1, d1, p2, d2), ...]: the candidates at list
    positions p1 and p2 are the query with exactly d1 and d2 bits flipped (p2 None: no second one); every other
    candidate is random (more than 80 bits from every query).  p2 = p1 + 64*m puts the pair in one lane of the
    wave-per-node kernels, anything else in two.  invalid: list positions whose c_valid is 0.
    -> scene as crowded_nodes (cv all 1 but `invalid`), queries at list position = index in pairs."""
    r = np.random.default_rng(seed)
    qd = r.integers(0, 256, (len(pairs), 32), dtype=np.uint8)
    cd = r.integers(0, 256, (nc, 32), dtype=np.uint8)
    used = set()
    for i, (p1, d1, p2, d2) in enumerate(pairs):
        for p, d in ((p1, d1), (p2, d2)):
            if p is None:
                continue
            assert 0 <= p < nc and p not in used, p
            used.add(p)
            cd[p] = _flip(r, qd[i], d)
    for i in range(len(pairs)):
        x = np.unpackbits(qd[i][None, :] ^ cd, axis=1).sum(1)
        mine = [p for p in (pairs[i][0], pairs[i][2]) if p is not None]
        x[mine] = 999
        assert x.min() > 80
    s = _scene(r, qd, cd, [0, len(pairs)], [0, nc])
    s["qa"] = np.zeros(len(pairs), np.float32); s["ca"] = np.zeros(nc, np.float32)
    s["qv"] = np.ones(len(pairs), np.uint8)
    s["cv"] = np.ones(nc, np.uint8); s["cv"][s["cit"][list(invalid)]] = 0
    return s


def singleton_nodes(angles_q, angles_c, seed=0, idle_q=0, idle_c=0):
    """One identical query and candidate per node (distance 0, no runner-up): every pair is accepted whatever the
    ratio, so angles_q[i] - angles_c[i] fixes the rotation histogram exactly.  idle_*: further features that belong
    to no node.  -> scene as crowded_nodes + pair_q / pair_c: the feature indices of pair i."""
    r = np.random.default_rng(seed)
    n = len(angles_q)
    d = r.integers(0, 256, (n, 32), dtype=np.uint8)
    s = _scene(r, d, d.copy(), np.arange(n + 1), np.arange(n + 1), idle_q, idle_c)
    s["qa"] = r.uniform(0, 360, n + idle_q).astype(np.float32); s["qa"][s["qit"]] = np.asarray(angles_q, np.float32)
    s["ca"] = r.uniform(0, 360, n + idle_c).astype(np.float32); s["ca"][s["cit"]] = np.asarray(angles_c, np.float32)
    s["qv"] = np.ones(n + idle_q, np.uint8); s["cv"] = np.ones(n + idle_c, np.uint8)
    s["pair_q"], s["pair_c"] = s["qit"].copy(), s["cit"].copy()
    return s


def merge(*scenes):
    """Scenes side by side: the nodes of each after those of the one before, feature indices shifted."""
    out = {k: [] for k in ("qd", "qa", "qv", "cd", "ca", "cv", "qit", "cit")}
    nqs, ncs, oq, oc = [0], [0], 0, 0
    for s in scenes:
        for k in ("qd", "qa", "qv", "cd", "ca", "cv"):
            out[k].append(s[k])
        out["qit"].append(s["qit"] + oq); out["cit"].append(s["cit"] + oc)
        nqs += [int(x) + nqs[-1] for x in np.diff(s["nqs"])]; ncs += [int(x) + ncs[-1] for x in np.diff(s["ncs"])]
        oq += len(s["qa"]); oc += len(s["ca"])
    out = {k: np.concatenate(v) for k, v in out.items()}
    out["qit"] = out["qit"].astype(np.int32); out["cit"] = out["cit"].astype(np.int32)
    out["nqs"], out["ncs"] = np.array(nqs, np.int32), np.array(ncs, np.int32)
    return out


def prefix(s, nnodes):
    """The first nnodes nodes of a scene (the item lists keep their length: the node offsets bound what is read)."""
    t = dict(s)
    t["nqs"], t["ncs"] = s["nqs"][:nnodes + 1], s["ncs"][:nnodes + 1]
    return t


# ---- the cases both test files run: built once per process, never modified ------------------------------------------
import functools
import itertools

FEATURE_COUNTS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 3001)    # group tails inside a wave, wave tails inside a block
# candidates / queries per node; prefixes of 1, 4, 5 and 9 nodes are run besides the whole list
CROWD_C = (64, 0, 65, 129, 4096, 63, 128, 1000, 4095, 10)
CROWD_Q = (40, 5, 80, 130, 150, 70, 64, 100, 150, 0)
CROWD_NNODES = (1, 4, 5, 9, 10)
VARIANTS = {"kf_frame": dict(use_cv=False, max_dist=50, strict=0),       # :159-288 bestDist1 <= TH_LOW, every candidate
            "kf_kf": dict(use_cv=True, max_dist=49, strict=1)}           # :522-655 bestDist1 <  TH_LOW, good map points only


@functools.lru_cache(None)
def descent_case(name):
    """-> (voc, feats[3001], paths): paths[i] = bow_ref.path(voc, feats[i]).  The wide vocabulary's probes are
    features 0..3, so every feature count holds at least one."""
    import bow_ref
    if name == "wide":
        rng = np.random.default_rng(5)
        voc = make_wide_vocabulary(rng)
        probes = np.stack([f for _, f, _ in voc["probes"]])
        feats = np.concatenate([probes, features_near_words(rng, voc, FEATURE_COUNTS[-1] - len(probes))])
    else:
        rng = np.random.default_rng(6)
        voc = make_vocabulary(rng, k=10, L=6, early_leaf=0.62)             # 24961 nodes, words at depths 2..6
        feats = features_near_words(rng, voc, FEATURE_COUNTS[-1])
    return voc, feats, [bow_ref.path(voc, f) for f in feats]


@functools.lru_cache(None)
def crowded_case():
    return crowded_nodes(CROWD_Q, CROWD_C, 9)


@functools.lru_cache(None)
def planted_case(max_dist):
    """planted_pairs for one SearchByBoW variant -> (scene, index): index[name] = the query feature indices of a
    group of planted pairs.  Node 0 (4096 candidates): the pairs; node 1: a sole candidate at distance 256; node 2:
    three near candidates that are all invalid."""
    pairs, index = [], {}

    def group(name, items):
        index[name] = list(range(len(pairs), len(pairs) + len(items)))
        pairs.extend(items)

    lane = itertools.cycle(range(64))
    def spot(m1, m2, other):                               # (p1, p2): rows m1, m2 of one lane, or of two lanes
        l1 = next(lane)
        return l1 + 64 * m1, (next(lane) if other else l1) + 64 * m2
    acc = lambda i: (8 + i, 2 * (8 + i) + 10)              # d1 < 0.7 * d2
    rej = lambda i: (30 - 3 * (i % 2), 40 - 4 * (i % 2))   # (30, 40), (27, 36): d1 == 0.75 * d2, accepted from 0.9 on
    group("same_lane", [(p1, acc(i)[0], p2, acc(i)[1]) for i in range(12) for p1, p2 in [spot(i % 5, i % 5 + 1 + i % 7, False)]])
    group("same_lane_below", [(p1, acc(i)[0], p2, acc(i)[1]) for i in range(4) for p1, p2 in [spot(9 + i, i, False)]])
    group("other_lane", [(p1, acc(i)[0], p2, acc(i)[1]) for i in range(10) for p1, p2 in [spot(i, 2 * i, True)]])
    group("same_lane_edge", [(p1, rej(i)[0], p2, rej(i)[1]) for i in range(4) for p1, p2 in [spot(i, 60 - i, False)]])
    group("other_lane_edge", [(p1, rej(i)[0], p2, rej(i)[1]) for i in range(2) for p1, p2 in [spot(3 * i, 7, True)]])
    group("tie_across", [(p1, 10 + i, p2, 10 + i) for i in range(10) for p1, p2 in [spot(i % 3, i % 3 + i % 2, True)]])
    group("tie_same_lane", [(p1, 20 + i, p2, 20 + i) for i in range(3) for p1, p2 in [spot(30 + i, 63 - i, False)]])
    group("at_max_dist", [(next(lane) + 64 * 63, max_dist, None, None)])
    group("over_max_dist", [(next(lane) + 64 * 2, max_dist + 1, None, None)])
    p1, p2 = spot(1, 40, True)
    group("invalid_runner_up", [(p1, 20, p2, 22)])
    assert len(pairs) == 48
    a = planted_pairs(pairs, 4096, 21, invalid=[p2])
    b = planted_pairs([(0, 256, None, None)], 1, 22)
    c = planted_pairs([(0, 5, 1, 9)], 3, 23, invalid=[0, 1, 2])
    s = merge(a, b, c)
    index = {k: [int(a["qit"][i]) for i in v] for k, v in index.items()}
    index["sole_256"] = [len(a["qa"]) + int(b["qit"][0])]
    index["all_invalid"] = [len(a["qa"]) + len(b["qa"]) + int(c["qit"][0])]
    return s, index


@functools.lru_cache(None)
def bow_reference(case, variant, ratio):
    """bow_ref.search_by_bow with the rotation filter on -> (nmatches, match_q, stats); stats["unfiltered"] and
    stats["accepted"] are the answer with the filter off."""
    import bow_ref
    v = VARIANTS[variant]
    s = crowded_case() if case == "crowded" else planted_case(v["max_dist"])[0]
    return bow_ref.search_by_bow(s["qd"], s["qa"], s["qv"], s["cd"], s["ca"], s["cv"] if v["use_cv"] else None, s["nqs"],
                                 s["qit"], s["ncs"], s["cit"], v["max_dist"], ratio, True)


def tri_geometry(s, seed, mono_only=False):
    """Keypoints for a crowded scene under a pure x-translation of 12 px (epipolar lines are the rows; F12 gives
    l = (0, 1, -y1)): features copied from one descriptor sit on one row up to noise.  -> dict(k1, f1, k2, f2, F12,
    ex, ey, sf, sigma2); the epipole lies inside the image so that the distance test bites."""
    r = np.random.default_rng(seed)
    ng = int(max(s["q_group"].max(), s["c_group"].max())) + 2
    gx, gy = r.uniform(20, 1220, ng), r.uniform(20, 356, ng)

    def kps(group, dx):
        n = len(group)
        k = np.zeros(n, KP_DTYPE)
        k["x"] = gx[group] + dx + r.normal(0, 0.3, n)
        k["y"] = gy[group] + r.normal(0, 0.8, n)
        k["octave"] = r.integers(0, 8, n)
        k["angle"] = (group * 0.5 + r.normal(0, 3, n)) % 360
        f = (r.random(n) > 0.2).astype(np.uint8) | ((r.random(n) < (0.0 if mono_only else 0.4)).astype(np.uint8) << 1)
        return k, f
    k1, f1 = kps(s["q_group"], 0.0)
    k2, f2 = kps(s["c_group"], -12.0)
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    return dict(k1=k1, f1=f1, k2=k2, f2=f2, F12=np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32), ex=600.0, ey=180.0,
                sf=sf, sigma2=(sf * sf).astype(np.float32))


@functools.lru_cache(None)
def tri_case():
    s = crowded_nodes(CROWD_Q, CROWD_C, 12, twins=0.5)
    return s, tri_geometry(s, 13)


@functools.lru_cache(None)
def tri_reference():
    import bow_ref
    s, g = tri_case()
    return bow_ref.search_for_triangulation(g["k1"], s["qd"], g["f1"], g["k2"], s["cd"], g["f2"], s["nqs"], s["qit"], s["ncs"],
                                            s["cit"], g["F12"], g["ex"], g["ey"], g["sf"], g["sigma2"], 50, True)


F12_ROWS = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)     # l = x1'F12 = (0, 1, -y1): den = 1, dsqr = (y2 - y1)^2


def singleton_tri(s, flags_q=3, flags_c=3):
    """Keypoints for a singleton_nodes scene: pair i on one row (the epipolar test passes with F12_ROWS), the angles of
    the scene, both stereo by default (no epipole test)."""
    nq, nc = len(s["qa"]), len(s["ca"])
    k1, k2 = np.zeros(nq, KP_DTYPE), np.zeros(nc, KP_DTYPE)
    k1["angle"], k2["angle"] = s["qa"], s["ca"]
    k1["x"], k2["x"] = 50.0, 40.0
    k1["y"][s["pair_q"]] = 20.0 + np.arange(len(s["pair_q"]))
    k2["y"][s["pair_c"]] = 20.0 + np.arange(len(s["pair_c"]))
    sf = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    return dict(k1=k1, f1=np.full(nq, flags_q, np.uint8), k2=k2, f2=np.full(nc, flags_c, np.uint8), F12=F12_ROWS.copy(), ex=600.0,
                ey=180.0, sf=sf, sigma2=(sf * sf).astype(np.float32))


@functools.lru_cache(None)
def orientation_cases():
    """Rotation histograms fixed pair by pair -> list of dict(name, scene, planted, hist, nmatches): planted = the
    distinct (q_angle, c_angle, bin) of the scene, hist the 30 bin sizes they must give, nmatches what survives.
    nq > 256 in every scene (k_bow_orient strides by 256); 260 query features belong to no node."""
    out = []

    def case(name, groups, survivors, valid=True):
        qa = np.concatenate([np.full(n, a, np.float32) for a, _, _, n in groups])
        ca = np.concatenate([np.full(n, c, np.float32) for _, c, _, n in groups])
        s = singleton_nodes(qa, ca, seed=len(out), idle_q=260, idle_c=7)
        hist = np.zeros(30, np.int64)
        for _, _, b, n in groups:
            hist[b] += n
        if not valid:
            s["qv"][:] = 0
            hist[:] = 0
        assert len(s["qa"]) > 256
        out.append(dict(name=name, scene=s, planted=[(np.float32(a), np.float32(c), b) for a, c, b, _ in groups], hist=hist,
                        nmatches=survivors))

    centre = lambda b, n: (30.0 * b + 7.0, 7.0, b, n)      # rot = 30 b exactly
    case("50_50_5", [centre(3, 50), centre(7, 50), centre(9, 5)], 105)            # 5 < 0.1f*50 is false: the third bin stays
    case("50_50_4", [centre(3, 50), centre(7, 50), centre(9, 4)], 100)
    case("10_10_1", [centre(3, 10), centre(7, 10), centre(9, 1)], 21)
    case("70_7_7", [centre(3, 70), centre(7, 7), centre(9, 7)], 84)
    case("70_6_6", [centre(3, 70), centre(7, 6), centre(9, 6)], 70)               # 6 < 7: the second and the third go
    case("four_equal", [centre(2, 30), centre(5, 30), centre(11, 30), centre(29, 30)], 90)   # the first three in bin order
    case("one_bin", [centre(4, 40)], 40)
    case("no_match", [centre(4, 40), centre(8, 9)], 0, valid=False)
    # edges: 10 pairs on the edge value + 30 in the middle of the bin they belong to, 35 each in bins 20 and 22: the bin
    # next door would come fourth (10 < 30), so a pair binned there is dropped and nmatches changes
    def edge(name, a, c, b):
        case(name, [(a, c, b, 10), centre(b, 30), centre(20, 35), centre(22, 35)], 110)
    for k in range(12):
        edge("edge_%d" % (30 * k + 15), 30.0 * k + 15.0, 0.0, k + 1)              # x.5 rounds away from zero
    edge("just_under_15", 14.99999, 0.0, 0)
    edge("minus_zero", -0.0, 0.0, 0)                                              # -0.0 < 0 is false: no wrap
    edge("wrap_350", 10.0, 20.0, 12)
    edge("wrap_to_360", 0.0, 1e-6, 12)                                            # -1e-6 + 360 rounds to 360
    edge("just_under_360", 359.99997, 0.0, 12)
    edge("bin_30", 900.0, 0.0, 0)                                                 # round(30.00..) == HISTO_LENGTH -> 0
    return out


def _pairs_tri(n, seed):
    s = singleton_nodes(np.zeros(n, np.float32), np.zeros(n, np.float32), seed=seed)
    g = singleton_tri(s, 1, 1)
    return s, g


@functools.lru_cache(None)
def tri_edge_cases():
    """-> list of dict(name, scene, geom, expect): expect[i] = whether pair i (query feature scene["pair_q"][i]) must
    match.  One query and one identical candidate per node, both monocular unless said otherwise."""
    f = np.float32
    up, dn = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    out = []
    # the epipole test `distex*distex+distey*distey < 100*scaleFactor[octave]` around exactly 10 px at octave 0
    spots = [(594, 172, 0, 1, 1, True), (up(594), 172, 0, 1, 1, False), (dn(594), 172, 0, 1, 1, True),
             (594, up(172), 0, 1, 1, False), (594, dn(172), 0, 1, 1, True),
             (up(594), 172, 0, 3, 1, True), (up(594), 172, 0, 1, 3, True), (up(594), 172, 0, 3, 3, True),   # a stereo side: no test
             (594, 172, 1, 1, 1, False),                                          # 100 < 100 * 1.2f
             (594, 172, 0, 0, 1, False), (594, 172, 0, 1, 0, False), (594, 172, 0, 2, 1, False)]            # unusable
    s, g = _pairs_tri(len(spots), 40)
    for i, (x, y, octave, fq, fc, _) in enumerate(spots):
        iq, ic = s["pair_q"][i], s["pair_c"][i]
        g["k2"]["x"][ic], g["k2"]["y"][ic], g["k2"]["octave"][ic] = x, y, octave
        g["k1"]["x"][iq], g["k1"]["y"][iq] = 300.0, y
        g["f1"][iq], g["f2"][ic] = fq, fc
    out.append(dict(name="epipole", scene=s, geom=g, expect=[e for *_, e in spots]))
    # dsqr < 3.84 * sigma2[octave] in double, dsqr = (y2 - y1)^2 in float: the last y2 that passes and the next float
    rows = []
    for octave in (0, 3, 7):
        limit = 3.84 * float(g["sigma2"][octave])
        y1 = f(100.0)
        passes = lambda y: float((y - y1) * (y - y1)) < limit
        y2 = f(y1 + f(np.sqrt(limit)) - f(1e-4))
        assert passes(y2) and not passes(f(y2 + f(2e-4)))
        while passes(up(y2)):
            y2 = up(y2)
        rows += [(y1, y2, octave, True), (y1, up(y2), octave, False), (y1, f(2 * y1 - y2), octave, True), (y1, dn(2 * y1 - y2), octave, False)]
    s, g = _pairs_tri(len(rows), 41)
    for i, (y1, y2, octave, _) in enumerate(rows):
        iq, ic = s["pair_q"][i], s["pair_c"][i]
        g["k1"]["y"][iq], g["k2"]["y"][ic], g["k2"]["octave"][ic] = y1, y2, octave
    g["f1"][:] = 3                                                                # stereo queries: no epipole test
    out.append(dict(name="dsqr", scene=s, geom=g, expect=[e for *_, e in rows]))
    # den = a*a + b*b == 0 -> false; a = F12(2,0), b = c = 0 and x2 = 0, so num = 0 and dsqr = 0 / den passes whenever den != 0
    for name, a, ok in (("den_zero", 0.0, False), ("den_underflows", 2.0 ** -75, False), ("den_subnormal", 2.0 ** -74, True),
                        ("den_smallest_normal", 2.0 ** -63, True)):
        s, g = _pairs_tri(3, 42)
        g["F12"] = np.zeros((3, 3), np.float32)
        g["F12"][2, 0] = a
        g["k2"]["x"][:] = 0.0
        g["f1"][:] = 3
        out.append(dict(name=name, scene=s, geom=g, expect=[ok] * 3))
    return out


# ---- helpers of both test files
def oracle_bow(oracle, s, variant, ratio, ori):
    v = VARIANTS[variant]
    return oracle.search_by_bow(s["qd"], s["qa"], s["qv"], s["cd"], s["ca"], s["cv"] if v["use_cv"] else None, s["nqs"], s["qit"],
                                s["ncs"], s["cit"], 50, v["strict"], ratio, ori)


def oracle_tri(oracle, s, g, ori, max_dist=50):
    return oracle.search_for_triangulation(g["k1"], s["qd"], g["f1"], g["k2"], s["cd"], g["f2"], s["nqs"], s["qit"], s["ncs"], s["cit"],
                                           g["F12"], g["ex"], g["ey"], g["sf"], g["sigma2"], max_dist, ori)


def descent_conditions(name):
    """What the features of a descent case reach, counted on the reference's paths."""
    voc, feats, paths = descent_case(name)
    late = sum(int(best >= 16) for _, steps in paths for best, _ in steps)
    stride_ties = sum(int(any(len(set(int(t) // 16 for t in tied)) > 1 for _, tied in steps)) for _, steps in paths)
    depths = sorted(set(len(nodes) for nodes, _ in paths))
    return late, stride_ties, depths


def planted_answers(variant, ratio):
    """How many queries of each planted group match (bow_scene.planted_case): (30, 40) and (27, 36) fail at 0.7 and at
    exactly 0.75, ties pass only above 1, max_dist itself passes and max_dist + 1 does not, distance 256 never does, an
    invalid candidate is neither a match nor a runner-up (20 vs 22 passes 0.7 and 0.9 only without the 22)."""
    kf = variant == "kf_kf"
    return dict(same_lane=12, same_lane_below=4, other_lane=10, same_lane_edge=4 * (ratio > 0.75), other_lane_edge=2 * (ratio > 0.75),
                tie_across=10 * (ratio > 1), tie_same_lane=3 * (ratio > 1), at_max_dist=1, over_max_dist=0,
                invalid_runner_up=int(kf or ratio > 1), sole_256=0, all_invalid=int(not kf))
