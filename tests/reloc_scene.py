"""Seeded synthetic worlds for the relocalisation chain (tests/reloc_chain.py): flat records, no images.

World.  Camera 640 x 480, K = 500 / 500 / 320 / 240, 8 levels of factor 1.2 (as tests/pnp_scene.py); a vocabulary from
bow_scene.make_vocabulary (k = 10, L = 3); one map; 5 or 6 keyframes; one query frame at a known true pose.

The query sees `core` map points (depth 3-9 in front of its true pose).  Each core point belongs to one GROUP, which decides how
the query's keypoint relates to it:
    near    the descriptor within 8 bits of the point's, keypoint = projection + pixel noise: SearchByBoW (TH_LOW 50) finds it
    wide    the descriptor 56-88 bits off: not for SearchByBoW, found by SearchByProjection(th 10, ORBdist 100)
    false   as wide, but the keypoint 4-8 level-pixels off its projection: found at th 10, an outlier of the next optimisation
    narrow  the descriptor 52-57 bits off and the keypoint's angle 5 histogram bins off: the rotation histogram of the th-10 search,
            full of `wide` matches in three other bins, throws it out; the th-3 / ORBdist-64 search, whose histogram holds the new
            matches only, keeps it.  This is how a point missed at 10 / 100 is found at 3 / 64.
The rest of the query's keypoints is clutter: random pixels, descriptors near words that no keyframe holds, so that clutter changes
neither the database's answer nor a match.

Every keyframe that is to become a candidate holds its own bit-flipped copy of ALL core descriptors, so the database ranks them
alike and answers them in id order; what they differ in is GetMapPointMatches:
    true    the entries are the map's core points (`keep` < 1: the others are null; `groups`: only these groups are kept)
    copy    the entries are the keyframe's own map points, the core positions moved by `pos_noise` (a badly triangulated copy),
            a share `junk` of them moved by about a unit
    decoy   own map points at unrelated positions: another place that looks the same
Some kept entries are set null and some map points bad (`null`, `bad_points`), and a keyframe may be bad itself.  Keyframes of
kind `other` see another place with other words and are no candidates.

BoW and feature vectors of every frame are the vocabulary's own transform(., 4) (with L = 3 every feature's node is the root, so
SearchByBoW compares all against all).  N <= 300 keypoints per frame.

SCENES names each scene for the branch of Tracking::Relocalization (src/Tracking.cc) it exists to reach, with the seed that
reaches it on the CPU chain (tests/test_reloc_chain_cpu.py asserts the branch; SEEDS_TRIED says how many seeds were looked at).
`narrow` IS reached - by construction, through the rotation histogram, not by chance."""
import numpy as np

import bow_scene

W, H = 640, 480
K = (500.0, 500.0, 320.0, 240.0)
CAM = (500.0, 500.0, 320.0, 240.0, 40.0, 0.08)          # fx fy cx cy mbf mb; the query is monocular, mbf / mb are never read
NLEVELS, SCALE = 8, 1.2
KP_DTYPE = bow_scene.KP_DTYPE
_cache = {}


def tables():
    """mvScaleFactor, mvLevelSigma2, mvInvLevelSigma2 as ORBextractor's constructor fills them (src/ORBextractor.cc:415-431)"""
    sf = [np.float32(1.0)]
    for _ in range(NLEVELS - 1):
        sf.append(np.float32(sf[-1] * np.float64(np.float32(SCALE))))
    sf = np.array(sf, np.float32)
    s2 = (sf * sf).astype(np.float32)
    return sf, s2, (np.float32(1.0) / s2).astype(np.float32)


SF, LEVEL_SIGMA2, INV_LEVEL_SIGMA2 = tables()
LOG_SF = np.float32(np.log(np.float32(SCALE)))


def rodrigues(axis, ang):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def pose(rng, ang, trans):
    T = np.eye(4)
    T[:3, :3] = rodrigues(rng.normal(size=3), ang)
    T[:3, 3] = rng.uniform(-trans, trans, 3)
    return T


def project(T, Xw):
    Xc = Xw @ T[:3, :3].T + T[:3, 3]
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1), Xc[:, 2]


def flip(rng, d, lo, hi):
    """each row of d with between lo and hi of its 256 bits flipped"""
    out = d.copy()
    for i in range(len(d)):
        f = np.zeros(256, np.uint8)
        f[rng.choice(256, int(rng.integers(lo, hi + 1)), replace=False)] = 1
        out[i] ^= np.packbits(f)
    return out


def keypoints(uv, level, angle):
    k = np.zeros(len(uv), KP_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"] = uv[:, 0], uv[:, 1], level, np.mod(angle, 360.0)
    k["size"], k["response"], k["class_id"] = 31.0 * SF[level], 50.0, -1
    return k


class Map:
    def __init__(self):
        self.pos, self.desc, self.normal, self.maxd, self.mind, self.bad, self.origin = [], [], [], [], [], [], []

    def add(self, pos, desc, Ow, level, origin=None):
        """map points seen from Ow at `level`: normal and distance range as MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:375-395).
        origin: the map point each one is a (moved) copy of; itself by default; -1: a point of another place"""
        i0 = len(self.pos)
        po = pos - Ow
        dist = np.linalg.norm(po, axis=1)
        for j in range(len(pos)):
            self.pos.append(pos[j]); self.desc.append(desc[j]); self.normal.append(po[j] / dist[j])
            self.maxd.append(dist[j] * SF[level[j]]); self.mind.append(dist[j] * SF[level[j]] / SF[NLEVELS - 1]); self.bad.append(False)
            self.origin.append(i0 + j if origin is None else int(origin[j]))
        return np.arange(i0, i0 + len(pos))

    def freeze(self):
        return dict(pos=np.array(self.pos, np.float32).reshape(-1, 3), desc=np.array(self.desc, np.uint8).reshape(-1, 32),
                    normal=np.array(self.normal, np.float32).reshape(-1, 3), maxd=np.array(self.maxd, np.float32),
                    mind=np.array(self.mind, np.float32), bad=np.array(self.bad, bool), origin=np.array(self.origin, np.int64))


def make(seed, groups, kfs, noise=0.5, clutter=60, wide_bins=(0, 1, 2), foreign_query=False):
    """groups: dict name -> count of core points.  kfs: list of dicts (kind, keep, groups, pos_noise, null, bad_points, bad, extra).
    foreign_query: the query's own descriptors are replaced by clutter descriptors (it shares no word with any keyframe)."""
    import oracle
    rng = np.random.default_rng(seed)
    voc = bow_scene.make_vocabulary(rng, k=10, L=3)
    ov = oracle.Vocabulary(voc["k"], voc["L"], 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    Tq = pose(rng, rng.uniform(0.1, 0.6), 2.0)
    Rq, tq = Tq[:3, :3], Tq[:3, 3]
    ncore = sum(groups.values())
    group = np.concatenate([np.full(c, g) for g, c in groups.items()]) if ncore else np.zeros(0, "<U8")
    # the core points, in front of the true pose
    z = rng.uniform(3, 9, ncore)
    u, v = rng.uniform(30, W - 30, ncore), rng.uniform(30, H - 30, ncore)
    Xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    Xw = (Xc - tq) @ Rq
    level = rng.integers(0, NLEVELS, ncore)
    base_angle = rng.uniform(0, 360, ncore)
    desc = bow_scene.features_near_words(rng, voc, ncore)
    m = Map()
    Oq = -Rq.T @ tq
    core_id = m.add(Xw, desc, Oq, level)
    # the query frame
    uvq = np.stack([u, v], axis=1) + rng.normal(0, 1, (ncore, 2)) * (noise * SF[level])[:, None]
    dq = desc.copy()
    ang_off = np.zeros(ncore)
    for g, (lo, hi) in (("near", (0, 8)), ("wide", (56, 88)), ("false", (56, 88)), ("narrow", (52, 57))):
        sel = np.nonzero(group == g)[0]
        dq[sel] = flip(rng, desc[sel], lo, hi)
    sel = np.nonzero(group == "false")[0]
    d = rng.normal(size=(len(sel), 2))
    uvq[sel] += d / np.linalg.norm(d, axis=1)[:, None] * (rng.uniform(4, 8, len(sel)) * SF[level[sel]])[:, None]
    for g in ("wide", "false"):
        sel = np.nonzero(group == g)[0]
        ang_off[sel] = 12.0 * np.asarray(wide_bins)[np.arange(len(sel)) % len(wide_bins)]
    ang_off[group == "narrow"] = 12.0 * 5
    ang_q = base_angle - ang_off + rng.uniform(-2, 2, ncore)          # rot = keyframe angle - frame angle (src/ORBmatcher.cc:1553)
    specs = []
    held = set()
    for ki, s in enumerate(kfs):
        kind = s["kind"]
        Tk = pose(rng, rng.uniform(0.02, 0.1), 0.4) @ Tq               # a keyframe near the query's true pose
        Ok = -Tk[:3, :3].T @ Tk[:3, 3]
        if kind == "other":
            n = s.get("n", 120)
            zz = rng.uniform(3, 9, n)
            pc = np.stack([(rng.uniform(30, W - 30, n) - K[2]) / K[0] * zz, (rng.uniform(30, H - 30, n) - K[3]) / K[1] * zz, zz], axis=1)
            far = pose(rng, 1.5, 30.0)
            Tk = far
            Ok = -Tk[:3, :3].T @ Tk[:3, 3]
            pw = (pc - Tk[:3, 3]) @ Tk[:3, :3]
            lv = rng.integers(0, NLEVELS, n)
            dk = bow_scene.features_near_words(rng, voc, n)
            mp = m.add(pw, dk, Ok, lv)
            uvk, ang_k = project(Tk, pw)[0] + rng.normal(0, 0.5, (n, 2)), rng.uniform(0, 360, n)
        else:
            n = ncore
            lv = level.copy()
            dk = flip(rng, desc, 0, 6)
            ang_k = base_angle + rng.uniform(-2, 2, n)
            if kind == "true":
                mp = core_id.copy()
                uvk = project(Tk, Xw)[0] + rng.normal(0, 1, (n, 2)) * (noise * SF[lv])[:, None]
            elif kind == "copy":
                pw = Xw + rng.normal(0, s.get("pos_noise", 0.05), (n, 3))
                junk = rng.random(n) < s.get("junk", 0.0)                # triangulated from a wrong match: anywhere near
                pw[junk] += rng.normal(0, 1.0, (int(junk.sum()), 3))
                mp = m.add(pw, desc, Ok, lv, origin=core_id)
                uvk = project(Tk, pw)[0]
            else:                                                      # decoy
                zz = rng.uniform(3, 9, n)
                pc = np.stack([(rng.uniform(30, W - 30, n) - K[2]) / K[0] * zz, (rng.uniform(30, H - 30, n) - K[3]) / K[1] * zz, zz], axis=1)
                Tk = pose(rng, 1.0, 20.0)
                Ok = -Tk[:3, :3].T @ Tk[:3, 3]
                pw = (pc - Tk[:3, 3]) @ Tk[:3, :3]
                mp = m.add(pw, desc, Ok, lv, origin=np.full(n, -1))
                uvk = project(Tk, pw)[0]
            keep = np.ones(n, bool)
            if "groups" in s:
                keep &= np.isin(group, s["groups"])
            if s.get("keep", 1.0) < 1.0:
                idx = np.nonzero(keep)[0]
                drop = rng.choice(idx, len(idx) - int(round(s["keep"] * len(idx))), replace=False)
                keep[drop] = False
            idx = np.nonzero(keep)[0]
            keep[rng.choice(idx, min(len(idx), s.get("null", 3)), replace=False)] = False         # GetMapPointMatches entries that are null
            mp = np.where(keep, mp, -1)
            idx = np.nonzero(keep)[0]
            for j in rng.choice(idx, min(len(idx), s.get("bad_points", 3)), replace=False):      # map points that are bad
                m.bad[mp[j]] = True
            extra = s.get("extra", 10)                                 # private keypoints without a map point
            if extra:
                dk = np.concatenate([dk, bow_scene.features_near_words(rng, voc, extra)])
                uvk = np.concatenate([uvk, np.stack([rng.uniform(0, W, extra), rng.uniform(0, H, extra)], axis=1)])
                lv = np.concatenate([lv, rng.integers(0, NLEVELS, extra)])
                ang_k = np.concatenate([ang_k, rng.uniform(0, 360, extra)])
                mp = np.concatenate([mp, np.full(extra, -1)])
        bw, bv, fv = ov.transform(dk, 4)
        held |= set(int(w) for w in bw)
        specs.append(dict(id=ki, kind=kind, Tcw=Tk.astype(np.float32), k=keypoints(uvk, lv, ang_k), d=np.ascontiguousarray(dk), mp=mp.astype(np.int64),
                          bow=list(zip([int(w) for w in bw], [float(x) for x in bv])), fv=fv, bad=bool(s.get("bad", False))))
    # clutter: descriptors near words that no keyframe holds
    cd = np.zeros((0, 32), np.uint8)
    want = clutter + (ncore if foreign_query else 0)
    while len(cd) < want:
        c = bow_scene.features_near_words(rng, voc, 2 * want)
        cw = np.array([ov.transform_one(x, 4)[0] for x in c])
        cd = np.concatenate([cd, c[~np.isin(cw, list(held))]])[:want]
    if foreign_query:
        dq = cd[clutter:]
        cd = cd[:clutter]
    uvc = np.stack([rng.uniform(0, W, clutter), rng.uniform(0, H, clutter)], axis=1)
    kq = np.concatenate([keypoints(uvq, level, ang_q), keypoints(uvc, rng.integers(0, NLEVELS, clutter), rng.uniform(0, 360, clutter))])
    dq = np.ascontiguousarray(np.concatenate([dq, cd]))
    perm = rng.permutation(len(kq))                                    # keypoint order says nothing about what a keypoint is
    kq, dq = kq[perm], dq[perm]
    planted = np.concatenate([core_id, np.full(clutter, -1)])[perm]
    grp = np.concatenate([group, np.full(clutter, "clutter")])[perm]
    bw, bv, fv = ov.transform(dq, 4)
    assert len(kq) <= 300 and all(len(s["k"]) <= 300 for s in specs)
    query = dict(k=kq, d=dq, bow=list(zip([int(w) for w in bw], [float(x) for x in bv])), fv=fv, Tcw_true=Tq, planted=planted, group=grp)
    nwords = int((voc["is_leaf"] == 1).sum())
    return dict(seed=seed, voc=voc, nwords=nwords, map=m.freeze(), kfs=specs, query=query)


TRUE = dict(kind="true")
OTHER = dict(kind="other")
DECOY = dict(kind="decoy")
# name -> (seed, constructor).  What each scene is for stands in tests/test_reloc_chain_cpu.py: EXPECT.
SCENES = {
    "direct": (1, lambda s: make(s, dict(near=130), [TRUE, OTHER, OTHER, OTHER], clutter=80)),
    "widen": (1, lambda s: make(s, dict(near=44, wide=60), [OTHER, TRUE, OTHER, OTHER], clutter=80)),
    "narrow": (1, lambda s: make(s, dict(near=26, wide=24, false=6, narrow=8), [OTHER, OTHER, TRUE, OTHER], clutter=80)),
    "decoy_first": (26, lambda s: make(s, dict(near=21, wide=70), [DECOY, dict(kind="copy", pos_noise=0.03), OTHER, OTHER, OTHER], noise=0.9, clutter=60)),
    "few_matches": (1, lambda s: make(s, dict(near=120), [dict(kind="true", keep=0.12), dict(kind="true", bad=True), TRUE, OTHER, OTHER], clutter=80)),
    "weak_pose": (176, lambda s: make(s, dict(near=20, wide=40), [dict(kind="copy", pos_noise=0.04), TRUE, OTHER, OTHER], noise=0.9, clutter=60)),
    "lost": (1, lambda s: make(s, dict(near=60), [DECOY, dict(kind="true", keep=0.15), DECOY, OTHER, OTHER], clutter=80)),
    "no_candidates": (1, lambda s: make(s, dict(near=80), [TRUE, OTHER, OTHER, OTHER], clutter=60, foreign_query=True)),
}
# seeds looked at on the CPU chain per scene -> (tried, of which reached the branch, kept).  decoy_first needs a candidate that is
# adopted, falls short of 50 and wins in a LATER pass with a new record set: 3 seeds in 400 (26 wins in pass 8, the longest).  weak_pose needs 11 PnP inliers of which
# the optimiser keeps 9: 8 seeds in 400 (seed 176 is the one whose weak candidate also stays alive).  narrow is reached by
# construction: 4 of the first 12 seeds, the others land one or two counts beside a threshold.
SEEDS_TRIED = {"direct": (1, 1, 1), "widen": (1, 1, 1), "narrow": (12, 4, 1), "decoy_first": (400, 3, 26), "few_matches": (1, 1, 1),
               "weak_pose": (400, 8, 176), "lost": (1, 1, 1), "no_candidates": (1, 1, 1)}


def scene(name, seed=None):
    key = (name, seed)
    if key not in _cache:
        s0, f = SCENES[name]
        sc = f(s0 if seed is None else seed)
        sc["name"] = name
        _cache[key] = sc
    return _cache[key]
