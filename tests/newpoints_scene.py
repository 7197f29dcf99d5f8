"""Seeded scenes for CreateNewMapPoints' per-match body: two keyframes that see the same world points, the matches between them,
and per row a reason to be accepted or to leave at one named test.  case(name) builds a scene; assert_conditions(name) checks, on the
restatement's own trace and before any comparison with a kernel, that the scene shows what it is named for and that no decision
sits where the device's atan2f / cosf (4 float steps either way, the project's allowance) or an equality could turn it.

A scene: {"kf1": keyframe, "kf2": keyframe, "pairs": [nm, 2] int32}; a keyframe: {"view", "kp", "st" (None: monocular), "sf", "sig2"}.
"""
import numpy as np

import newpoints_ref as R

F32, F64 = np.float32, np.float64
NLEVELS, SCALE = 8, 1.2
SF = np.array([SCALE ** l for l in range(NLEVELS)], F32)
SIG2 = (SF * SF).astype(F32)
K = (500.0, 500.0, 320.0, 240.0)
MB, MBF = 0.1, 50.0
FAULTS = ["behind1", "behind2", "reproj1", "reproj2", "scale", "lowpar"]


def _pose(ry, C):
    """Tcw of a camera at C turned by ry about the world's y axis"""
    c, s = np.cos(ry), np.sin(ry)
    Rcw = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rcw, -Rcw @ np.asarray(C, F64)
    return T


def _project(T, X):
    Xc = X @ T[:3, :3].T + T[:3, 3]
    return K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3], Xc[:, 2]


def make(seed, nm, kind1="mono", kind2="mono", baseline=0.6, faults=True, mbf2=MBF, raw_shift=0.0, extra=(7, 5)):
    """kind: "mono" (no stereo array), "stereo" (every feature stereo), "mixed" (a stereo array, ur < 0 on about half)"""
    rng = np.random.default_rng(seed)
    T1 = _pose(0.0, (0, 0, 0))
    C2 = np.array([baseline, -0.02 * baseline / 0.6, 0.3 * baseline / 0.6])
    T2 = _pose(0.05 * baseline / 0.6, C2)
    X = np.stack([rng.uniform(-2, 2, nm), rng.uniform(-1.2, 1.2, nm), rng.uniform(3, 9, nm)], axis=1)
    kind = np.array(["ok"] * nm, dtype=object)
    if faults and nm >= 16:
        pick = rng.permutation(nm)[:max(len(FAULTS), nm // 5)]
        for j, r in enumerate(pick):
            kind[r] = FAULTS[j % len(FAULTS)]
    n1, n2 = nm + extra[0], nm + extra[1]
    idx1, idx2 = rng.permutation(n1)[:nm], rng.permutation(n2)[:nm]
    mono1 = np.ones(n1, bool) if kind1 == "mono" else (np.zeros(n1, bool) if kind1 == "stereo" else rng.random(n1) < 0.5)
    mono2 = np.ones(n2, bool) if kind2 == "mono" else (np.zeros(n2, bool) if kind2 == "stereo" else rng.random(n2) < 0.5)
    for r in range(nm):
        if kind[r] == "behind1":
            X[r, 2] = -X[r, 2]
        elif kind[r] == "behind2":                 # in front of keyframe 1, behind keyframe 2 (which stands 0.3 further along z)
            X[r] = [rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01), rng.uniform(0.05, 0.2) * baseline / 0.6]
        elif kind[r] == "lowpar":                  # only a pair of monocular features can fail on parallax alone
            if mono1[idx1[r]] and mono2[idx2[r]]:
                X[r, 2] = rng.uniform(300, 500)
            else:
                kind[r] = "ok"
    u1, v1, z1 = _project(T1, X)
    u2, v2, z2 = _project(T2, X)
    o1 = rng.integers(0, 4, nm)
    d1, d2 = np.linalg.norm(X, axis=1), np.linalg.norm(X - C2, axis=1)
    o2 = np.clip(o1 + np.round(np.log(d2 / d1) / np.log(SCALE)).astype(int), 0, NLEVELS - 1)
    noise = rng.normal(0, 0.25, (nm, 6))
    for r in range(nm):
        if kind[r] == "reproj1":
            noise[r, 1] += 12.0; o1[r] = 0; o2[r] = 0
        elif kind[r] == "reproj2":
            noise[r, 4] += 12.0; o1[r] = 7; o2[r] = 0
        elif kind[r] == "scale":
            o1[r] = 0; o2[r] = 7

    def keyframe(T, n, idx, u, v, z, o, mono, mbf, nz):
        kp = np.zeros(n, R.KP_DTYPE)
        kp["x"], kp["y"] = rng.uniform(20, 620, n), rng.uniform(20, 460, n)
        kp["octave"] = rng.integers(0, NLEVELS, n)
        kp["x"][idx], kp["y"][idx], kp["octave"][idx] = u + nz[:, 0], v + nz[:, 1], o
        kp["size"], kp["angle"] = 31.0, rng.uniform(0, 360, n)
        st = None
        if not mono.all():
            st = np.zeros(n, R.STEREO_DTYPE)
            zz = rng.uniform(3, 9, n)
            zz[idx] = np.abs(z)
            ur = kp["x"].astype(F64) - mbf / zz
            ur[idx] += nz[:, 2]
            st["ur"] = ur
            with np.errstate(all="ignore"):
                st["depth"] = F32(mbf) / (kp["x"] - st["ur"])      # as Frame::ComputeStereoMatches forms it: mbf / disparity, float
            st["raw_u"], st["raw_v"] = kp["x"] + F32(raw_shift), kp["y"] - F32(raw_shift) * F32(0.5)
            bad = mono | ~(st["depth"] > 0)
            st["ur"][bad], st["depth"][bad] = -1, -1
        return {"view": R.view(T, K, MB, mbf, SCALE, NLEVELS), "kp": kp, "st": st, "sf": SF.copy(), "sig2": SIG2.copy()}

    kf1 = keyframe(T1, n1, idx1, u1, v1, z1, o1, mono1, MBF, noise[:, 0:3])
    kf2 = keyframe(T2, n2, idx2, u2, v2, z2, o2, mono2, mbf2, noise[:, 3:6])
    return {"kf1": kf1, "kf2": kf2, "pairs": np.stack([idx1, idx2], axis=1).astype(np.int32), "kind": kind, "X": X}


def _wzero():
    """w == 0 on purpose: two 'rotations' that are no rotations, whose first columns are the keypoints' own rays, so that column 0 of A
    is exactly zero, the null vector is e_0 and the rays still differ (cos 0.6)"""
    sc = make(901, 1, faults=False, extra=(0, 0))
    for kf, h in ((sc["kf1"], 0.5), (sc["kf2"], -0.5)):
        T = np.eye(4, dtype=F32)
        T[:3, :3] = [[0, 1, 0], [0, 0, 1], [1, h, 0]]
        T[:3, 3] = [0.25 + h, -0.5 - h, 2.0]
        kf["view"]["Tcw"] = T.reshape(16)
        kf["kp"]["x"], kf["kp"]["y"] = K[2], K[3]
    return sc


def _zero_dist():
    """dist1 == 0 on purpose: a point unprojected from keyframe 2's stereo feature, and keyframe 1's stored centre put onto it"""
    sc = make(902, 4, "mono", "stereo", baseline=0.03, faults=False)
    rows, _ = ref(sc)
    assert rows["status"][0] == 2
    sc["kf1"]["view"]["Ow"] = [rows["x"][0], rows["y"][0], rows["z"][0]]
    return sc


CASES = {
    "n0": lambda: make(100, 0, "mixed", "mixed"), "n1": lambda: make(101, 1, "mixed", "mixed"), "n63": lambda: make(163, 63, "mixed", "mixed"),
    "n64": lambda: make(164, 64, "mixed", "mixed"), "n65": lambda: make(165, 65, "mixed", "mixed"), "n255": lambda: make(355, 255, "mixed", "mixed"),
    "n256": lambda: make(356, 256, "mixed", "mixed"), "n257": lambda: make(357, 257, "mixed", "mixed"),
    "mono_mono": lambda: make(1, 96), "stereo_mono": lambda: make(2, 70, "stereo", "mono"), "mono_stereo": lambda: make(3, 70, "mono", "stereo"),
    "stereo_stereo": lambda: make(4, 70, "stereo", "stereo"),
    "near_stereo_stereo": lambda: make(5, 40, "stereo", "stereo", baseline=0.03, faults=False),     # the `else if` of :321
    "near_stereo_mono": lambda: make(6, 40, "stereo", "mono", baseline=0.03, faults=False),
    "near_mono_stereo": lambda: make(7, 40, "mono", "stereo", baseline=0.03, faults=False),
    "mbf_differs": lambda: make(8, 40, "stereo", "stereo", mbf2=15.0, faults=False),                # :414
    "raw_differs": lambda: make(9, 40, "stereo", "stereo", baseline=0.03, faults=False, raw_shift=1.5),   # mvKeys, not mvKeysUn
    "wzero": _wzero, "zero_dist": _zero_dist,
}
NOMINAL = ["n63", "n64", "n65", "n255", "n256", "n257", "mono_mono", "stereo_mono", "mono_stereo", "stereo_stereo", "near_stereo_stereo",
           "near_stereo_mono", "near_mono_stereo", "raw_differs"]
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def args(sc):
    a, b = sc["kf1"], sc["kf2"]
    return (a["view"], a["kp"], a["st"], a["sf"], a["sig2"], b["view"], b["kp"], b["st"], b["sf"], b["sig2"], sc["pairs"])


def ref(sc, **kw):
    return R.triangulate(*args(sc), **kw)


_refs = {}


def reference(name):
    """the restatement's rows and trace for a named scene, computed once and shared"""
    if name not in _refs:
        _refs[name] = ref(case(name))
    return _refs[name]


BATCH = ["mono_mono", "n0", "stereo_mono", "n65"]      # an empty pair second; offsets 0, 96, 96, 166, 231: no multiple of 64


def assert_conditions(name):
    sc = case(name)
    rows, tr = reference(name)
    st = rows["status"]
    nm = len(st)
    # 4 float steps either way on atan2f's and on cosf's result turn no decision
    for a in (-4, 0, 4):
        for c in (-4, 0, 4):
            r2, _ = ref(sc, shift=(a, c))
            assert (r2["status"] == st).all(), (name, a, c)
            for f in ("x", "y", "z", "cos_rays"):
                assert r2[f].tobytes() == rows[f].tobytes(), (name, a, c, f)
    # no other comparison sits on equality (w == 0 is listed with an empty `reached`; the two special scenes put theirs on purpose)
    for cname, lhs, rhs, reached in tr["cmp"]:
        if "cosStereo" in cname:
            continue
        assert not (reached & (lhs == rhs)).any(), (name, cname)
    if name in NOMINAL:
        assert 2 * (st >= 0).sum() >= nm, (name, np.unique(st, return_counts=True))
    if name in ("mono_mono", "n257"):
        assert (st == 0).sum() >= nm // 2
    if name == "mono_mono":
        assert set(st) >= {0, -1, -3, -4, -5, -6, -8}, set(st)
    if name == "near_stereo_stereo":      # both features stereo: only keyframe 1's angle is formed, so keyframe 2 can never be the one unprojected
        assert (st == 1).sum() >= nm // 2 and not (st == 2).any()
    if name == "near_stereo_mono":
        assert (st == 1).sum() >= nm // 2
    if name == "near_mono_stereo":
        assert (st == 2).sum() >= nm // 2
    if name == "stereo_stereo":
        assert (st == 0).sum() >= nm // 2
    if name == "mbf_differs":             # with keyframe 2's own mbf in :414 the rows would have been accepted
        assert (st == -6).sum() >= nm // 2
        r2, _ = ref(sc, own_mbf2=True)
        assert ((r2["status"] >= 0) & (st == -6)).sum() >= nm // 2
    if name == "raw_differs":             # the unprojected points move when the raw keypoint is replaced by the undistorted one
        k1 = dict(sc["kf1"], st=sc["kf1"]["st"].copy())
        k1["st"]["raw_u"], k1["st"]["raw_v"] = sc["kf1"]["kp"]["x"], sc["kf1"]["kp"]["y"]
        r2, _ = ref(dict(sc, kf1=k1))
        m = st == 1
        assert m.sum() >= nm // 2 and (np.abs(r2["x"][m] - rows["x"][m]) > 1e-3).all()
    if name == "wzero":
        assert list(st) == [-2] and rows["x"][0] == 0
    if name == "zero_dist":
        assert st[0] == -7 and tr["dist"][0][0] == 0 and rows["z"][0] != 0


def assert_every_status_occurs():
    seen = set()
    for name in CASES:
        seen |= set(int(s) for s in reference(name)[0]["status"])
    assert seen >= set(range(-8, 3)), sorted(seen)


# ------------------------------------------------------------------------------------------------------------------ the chain
def make_chain(seed, npts, centres, kinds, monocular, medians, nvis=0.7):
    """The current keyframe (kinds[0]) sees every point; neighbour i stands at centres[i] and sees about nvis of them.  Descriptors are
    the points' own with a few bits flipped, so only true correspondences come within TH_LOW; a point's vocabulary node is p % nnodes.
    A fifth of the points neighbours 0 and 1 share carry an octave in neighbour 0 that fails the scale test there (b)."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, npts), rng.uniform(-1.2, 1.2, npts), rng.uniform(3, 9, npts)], axis=1)
    pdesc = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    nnodes = max(4, npts // 3)
    o_cur = rng.integers(0, 4, npts)
    nn = len(centres)
    vis = [rng.random(npts) < nvis for _ in range(nn)]
    both = np.flatnonzero(vis[0] & vis[1]) if nn > 1 else np.zeros(0, np.int64)
    wrong_scale = both[::5]
    o_cur[wrong_scale] = 0

    def keyframe(T, C, pts, kind, extras, octs):
        n = len(pts) + extras
        idx = rng.permutation(n)[:len(pts)]
        u, v, z = _project(T, X[pts])
        nz = rng.normal(0, 0.25, (len(pts), 3))
        kp = np.zeros(n, R.KP_DTYPE)
        kp["x"], kp["y"], kp["octave"] = rng.uniform(20, 620, n), rng.uniform(20, 460, n), rng.integers(0, NLEVELS, n)
        kp["x"][idx], kp["y"][idx], kp["octave"][idx] = u + nz[:, 0], v + nz[:, 1], octs
        kp["size"], kp["angle"] = 31.0, rng.uniform(0, 360, n)
        mono = np.ones(n, bool) if kind == "mono" else rng.random(n) < 0.5
        st = None
        if kind != "mono":
            st = np.zeros(n, R.STEREO_DTYPE)
            zz = rng.uniform(3, 9, n)
            zz[idx] = z
            ur = kp["x"].astype(F64) - MBF / zz
            ur[idx] += nz[:, 2]
            st["ur"] = ur
            st["depth"] = F32(MBF) / (kp["x"] - st["ur"])
            st["raw_u"], st["raw_v"] = kp["x"], kp["y"]
            st["ur"][mono], st["depth"][mono] = -1, -1
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        d = pdesc[pts].copy()
        for r in range(len(pts)):
            for bit in rng.integers(0, 256, 5):
                d[r, bit >> 3] ^= np.uint8(1 << (bit & 7))
        desc[idx] = d
        node = rng.integers(0, nnodes, n)
        node[idx] = pts % nnodes
        flags = np.where(mono, 1, 3).astype(np.uint8)
        flags[rng.permutation(n)[:5]] &= 2                      # five features that already have a map point
        return ({"view": R.view(T, K, MB, MBF, SCALE, NLEVELS), "kp": kp, "st": st, "sf": SF.copy(), "sig2": SIG2.copy()}, desc, flags, node, idx)

    allp = np.arange(npts)
    cur, qd, qf, qnode, qidx = keyframe(_pose(0.0, (0, 0, 0)), np.zeros(3), allp, kinds[0], 9, o_cur)
    nbs, nodes = [], [qnode]
    for i in range(nn):
        C = np.asarray(centres[i], F64)
        T = _pose(0.04 * C[0], C)
        pts = np.flatnonzero(vis[i])
        d1, d2 = np.linalg.norm(X[pts], axis=1), np.linalg.norm(X[pts] - C, axis=1)
        octs = np.clip(o_cur[pts] + np.round(np.log(d2 / d1) / np.log(SCALE)).astype(int), 0, NLEVELS - 1)
        if i == 0:
            octs[np.isin(pts, wrong_scale)] = NLEVELS - 1
        kf, cd, cf, cnode, _ = keyframe(T, C, pts, kinds[1 + i], 6, octs)
        nodes.append(cnode)
        nqs, qi, ncs, ci = [0], [], [0], []
        for j in range(nnodes):
            a, b = np.flatnonzero(qnode == j), np.flatnonzero(cnode == j)
            if len(a) and len(b):
                qi += list(a); ci += list(b); nqs.append(len(qi)); ncs.append(len(ci))
        Tw, T1 = T.astype(F32), cur["view"]["Tcw"].reshape(4, 4)
        # the epipole as ORBmatcher::SearchForTriangulation forms it (src/ORBmatcher.cc:663-670): C2 = R2w*Cw + t2w a gemm, the rest in float
        Cc = R._mv(Tw[:3, :3], cur["view"]["Ow"].reshape(1, 3), Tw[:3, 3]).reshape(3)
        invz = F32(1.0) / Cc[2]
        nbs.append({"kf": kf, "cd": cd, "cf": cf, "nqs": np.array(nqs, np.int32), "qi": np.array(qi, np.int32), "ncs": np.array(ncs, np.int32),
                    "ci": np.array(ci, np.int32), "F12": R.compute_f12(T1, K, Tw, K), "ex": F32(K[0]) * Cc[0] * invz + F32(K[2]),
                    "ey": F32(K[1]) * Cc[1] * invz + F32(K[3]), "median": F32(medians[i])})
    return {"cur": cur, "qd": qd, "qf": qf, "nbs": nbs, "monocular": monocular, "node": nodes}


CHAINS = {
    # neighbour 2 stands 3 cm away: less than mb, the stereo baseline rule skips it (c)
    "chain_stereo": lambda: make_chain(31, 300, [(0.6, -0.02, 0.3), (-0.5, 0.03, 0.2), (0.03, 0.0, 0.0)], ["mixed"] * 4, False, [0, 0, 0]),
    # monocular: the rule is baseline / median depth; neighbour 1's median depth of 90 m makes 0.58 m too short
    "chain_mono": lambda: make_chain(32, 280, [(0.6, -0.02, 0.3), (-0.5, 0.03, 0.3), (0.4, 0.3, 0.1)], ["mono"] * 4, True, [6.0, 90.0, 5.5]),
}


def chain(name):
    if name not in _cache:
        _cache[name] = CHAINS[name]()
    return _cache[name]


def chain_ref(sc, **kw):
    return R.create_new_map_points(sc["cur"], sc["qd"], sc["qf"], sc["nbs"], sc["monocular"], **kw)


def chain_reference(name):
    if name not in _refs:
        _refs[name] = chain_ref(chain(name))
    return _refs[name]


def assert_chain_conditions(name):
    import bow_ref
    sc, r = chain(name), chain_reference(name)
    cur, nbs = sc["cur"], sc["nbs"]
    st = r["points"]["status"]
    for a in (-4, 4):
        for c in (-4, 4):
            r2 = chain_ref(sc, shift=(a, c))
            assert (r2["points"]["status"] == st).all() and (r2["match_q"] == r["match_q"]).all() and (r2["q_flags"] == r["q_flags"]).all()
    live = [i for i in range(len(nbs)) if not r["skipped"][i]]
    assert len(live) >= 2 and len(cur["kp"]) > 256
    for i in live:
        assert r["nmatches"][i] >= 40 and 2 * r["nnew"][i] >= r["nmatches"][i], (name, i, r["nmatches"], r["nnew"])
    i0, i1 = live[0], live[1]
    # (a) a query the first live neighbour accepted would also have matched in the next one, had its flag not been cleared
    nb = nbs[i1]
    _, fresh, _ = bow_ref.search_for_triangulation(cur["kp"], sc["qd"], sc["qf"], nb["kf"]["kp"], nb["cd"], nb["cf"], nb["nqs"], nb["qi"], nb["ncs"],
                                                   nb["ci"], nb["F12"], nb["ex"], nb["ey"], nb["kf"]["sf"], nb["kf"]["sig2"], 50, False)
    a = (st[i0] >= 0) & (fresh >= 0)
    assert a.sum() >= 5 and (r["match_q"][i1][a] == -1).all()
    # (b) a query matched but REJECTED by the first is matched and accepted by the next
    b = (r["match_q"][i0] >= 0) & (st[i0] < 0) & (st[i1] >= 0)
    assert b.sum() >= 3
    assert ((r["q_flags"] & 1) == ((sc["qf"] & 1) & ~(st >= 0).any(0))).all()
    if name == "chain_stereo":
        assert list(r["skipped"]) == [False, False, True] and (st[2] == -9).all()      # (c)
    if name == "chain_mono":
        assert list(r["skipped"]) == [False, True, False]
        assert R.baseline_ok(cur["view"], nbs[1]["kf"]["view"], True, 6.0)              # it is the median depth that skips it
