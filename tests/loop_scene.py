"""Seeded synthetic worlds for the loop-closing chain (tests/loop_chain.py): flat records, no images.

Camera, levels and vocabulary are reloc_scene's (640 x 480, K = 500 / 500 / 320 / 240, 8 levels of 1.2, make_vocabulary(k = 10, L = 3)).

A world has the two sides of a loop.
  LOOP SIDE (map frame W, keyframe ids < 10): a PLACE is a set of core map points in front of a pose; old keyframes near that pose see
  them.  Kinds of keyframe, as in reloc_scene:
      true    GetMapPointMatches holds the place's core points themselves (shared between keyframes: what mnLoopPointForKF de-duplicates)
      copy    own map points, the core positions moved by `pos_noise`; the points of group `bias` moved sideways by `bias` level-pixels
      decoy   own map points at unrelated positions: another place that looks the same
      other   another place with other words
  `holds`: the groups whose keypoints the keyframe has at all (its words); `groups`: those whose table entry is a map point.  Some kept
  entries are null, some points bad, a keyframe may be bad.  `conn` is its covisibility list (GetVectorCovisibleKeyFrames, at most 10,
  which is also GetBestCovisibilityKeyFrames(10) and, as a set, GetConnectedKeyFrames).
  CURRENT SIDE (map frame W' = S_d W, ids >= 10): recent keyframes that see a place again.  Their map points are copies of the place's
  core points under the similarity S_d (scale `scale`; 1 with fix_scale) plus position noise; their poses are rigid in W', so that
  Scw_true = T_iw' S_d maps the loop side's points into keyframe i.  sc["run"] are the keyframes LoopClosing processes in order; each is
  connected to every earlier current-side keyframe (so none of them is a candidate); keyframe 10 sees 40 % of the place, which makes it
  the lowest-scoring neighbour: the minimum score.

The descriptor GROUP of a core point says how the current side's keypoint relates to it:
    near    within 8 bits: found by SearchByBoW(current, candidate)
    wide    56-84 bits off: not for SearchByBoW (TH_LOW), found by SearchBySim3 at 7.5 (TH_HIGH)
    far     within 8 bits but seen only by the matched keyframe's NEIGHBOURS: found by SearchByProjection(Scw, 10) over the loop points
    bias    as wide, seen by a copy keyframe whose points are moved sideways: SearchBySim3 finds them and the refine stage's fit is bent
The rest of a keyframe's keypoints is clutter near words no other keyframe holds.

SCENES names each scene for the branch of LoopClosing (src/LoopClosing.cc) it must reach; tests/test_loop_chain_cpu.py asserts it
(EXPECT).  SEEDS_TRIED: per scene (seeds looked at on the CPU chain, of which reached the branch and met the conditions, kept)."""
import numpy as np

import bow_scene
from reloc_scene import CAM, H, K, KP_DTYPE, LEVEL_SIGMA2, INV_LEVEL_SIGMA2, LOG_SF, NLEVELS, SF, W, Map, flip, keypoints, pose, project  # noqa: F401

_cache = {}
FLIPS = dict(near=(0, 8), wide=(56, 84), far=(0, 8), bias=(56, 84))


def backproject(rng, n, T):
    """n points at depth 3-9 inside the image of the camera at pose T (world -> camera) -> world positions"""
    z = rng.uniform(3, 9, n)
    u, v = rng.uniform(30, W - 30, n), rng.uniform(30, H - 30, n)
    Xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
    return (Xc - T[:3, 3]) @ T[:3, :3]


def clutter(rng, voc, ov, held, n):
    """n descriptors near words that are not in `held`"""
    cd = np.zeros((0, 32), np.uint8)
    while len(cd) < n:
        c = bow_scene.features_near_words(rng, voc, 2 * n + 8)
        cw = np.array([ov.transform_one(x, 4)[0] for x in c])
        cd = np.concatenate([cd, c[~np.isin(cw, list(held))]])[:n]
    return cd


def make(seed, places, loop, run, scale=1.08, fix_scale=False, last_loop=0, foreign=(), sees=None, noise=0.5, nclutter=50, pos_noise=0.004,
         bad_current=()):
    """places: list of dict group -> count.  loop: list of keyframe specs (id, kind, place, holds, groups, conn, keep, null, bad_points, bad,
    pos_noise, junk, bias).  run: the current keyframes LoopClosing processes.  sees: current id -> place (default 0).  foreign: current ids
    that see nothing any other keyframe holds."""
    import oracle
    rng = np.random.default_rng(seed)
    voc = bow_scene.make_vocabulary(rng, k=10, L=3)
    ov = oracle.Vocabulary(voc["k"], voc["L"], 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    sees = dict(sees or {})
    m = Map()
    P = []                                                             # per place: pose, core ids, groups, levels, angles, descriptors
    for pi, groups in enumerate(places):
        Tq = pose(rng, rng.uniform(0.1, 0.6), 2.0) if pi == 0 else pose(rng, 1.0, 20.0)
        n = sum(groups.values())
        Xw = backproject(rng, n, Tq)
        level, angle = rng.integers(0, NLEVELS, n), rng.uniform(0, 360, n)
        desc = bow_scene.features_near_words(rng, voc, n)
        ids = m.add(Xw, desc, -Tq[:3, :3].T @ Tq[:3, 3], level)
        P.append(dict(Tq=Tq, ids=ids, Xw=Xw, level=level, angle=angle, desc=desc, group=np.concatenate([np.full(c, g) for g, c in groups.items()])))
    kfs, held = {}, set()

    def finish(kid, Tk, uv, lv, ang, dk, mp, planted, conn, bad):
        bw, bv, fv = ov.transform(dk, 4)
        held.update(int(w) for w in bw)
        assert len(uv) <= 300
        kfs[kid] = dict(id=kid, Tcw=Tk.astype(np.float32), k=keypoints(uv, lv, ang), d=np.ascontiguousarray(dk), mp=np.asarray(mp, np.int64),
                        planted=np.asarray(planted, np.int64), bow=list(zip([int(w) for w in bw], [float(x) for x in bv])), fv=fv, bad=bool(bad),
                        conn=[int(c) for c in conn])

    # ---- the loop side
    for s in loop:
        kind, pl = s["kind"], P[s.get("place", 0)]
        n = len(pl["ids"])
        Tk = pose(rng, rng.uniform(0.02, 0.06), 0.15) @ pl["Tq"]
        Ok = -Tk[:3, :3].T @ Tk[:3, 3]
        if kind == "other":
            n = s.get("n", 100)
            Tk = pose(rng, 1.5, 30.0)
            pw = backproject(rng, n, Tk)
            lv, ang, dk = rng.integers(0, NLEVELS, n), rng.uniform(0, 360, n), bow_scene.features_near_words(rng, voc, n)
            mp = m.add(pw, dk, -Tk[:3, :3].T @ Tk[:3, 3], lv, origin=np.full(n, -1))
            finish(s["id"], Tk, project(Tk, pw)[0] + rng.normal(0, 0.5, (n, 2)), lv, ang, dk, mp, np.full(n, -1), s.get("conn", []), s.get("bad", False))
            continue
        lv, dk, ang = pl["level"].copy(), flip(rng, pl["desc"], 0, 6), pl["angle"] + rng.uniform(-2, 2, n)
        if kind == "true":
            mp = pl["ids"].copy()
            uv = project(Tk, pl["Xw"])[0] + rng.normal(0, 1, (n, 2)) * (noise * SF[lv])[:, None]
        elif kind == "copy":
            pw = pl["Xw"] + rng.normal(0, s.get("pos_noise", 0.02), (n, 3))
            junk = rng.random(n) < s.get("junk", 0.0)
            pw[junk] += rng.normal(0, 1.0, (int(junk.sum()), 3))
            sel = pl["group"] == "bias"                              # moved sideways in the keyframe's own image by `bias` level-pixels
            if sel.any():
                Xc = pw[sel] @ Tk[:3, :3].T + Tk[:3, 3]
                Xc[:, 0] += s.get("bias", 6.0) * SF[lv[sel]] * Xc[:, 2] / K[0]
                pw[sel] = (Xc - Tk[:3, 3]) @ Tk[:3, :3]
            mp = m.add(pw, pl["desc"], Ok, lv, origin=pl["ids"])
            uv = project(Tk, pw)[0] + rng.normal(0, 1, (n, 2)) * (0.3 * SF[lv])[:, None]
        else:                                                          # decoy
            Tk = pose(rng, 1.0, 20.0)
            pw = backproject(rng, n, Tk)
            mp = m.add(pw, pl["desc"], -Tk[:3, :3].T @ Tk[:3, 3], lv, origin=np.full(n, -1))
            uv = project(Tk, pw)[0]
        keep = np.isin(pl["group"], s["groups"]) if "groups" in s else np.ones(n, bool)
        if s.get("keep", 1.0) < 1.0:
            idx = np.nonzero(keep)[0]
            keep[rng.choice(idx, len(idx) - int(round(s["keep"] * len(idx))), replace=False)] = False
        idx = np.nonzero(keep)[0]
        keep[rng.choice(idx, min(len(idx), s.get("null", 3)), replace=False)] = False           # entries that are null
        mp = np.where(keep, mp, -1)
        idx = np.nonzero(keep)[0]
        for j in rng.choice(idx, min(len(idx), s.get("bad_points", 2)), replace=False):        # map points that are bad
            m.bad[mp[j]] = True
        has = np.isin(pl["group"], s["holds"]) if "holds" in s else np.ones(n, bool)            # the keypoints the keyframe has at all
        uv, lv, ang, dk, mp, planted = uv[has], lv[has], ang[has], dk[has], mp[has], pl["ids"][has]
        extra = s.get("extra", 10)                                     # private keypoints without a map point
        if extra:
            dk = np.concatenate([dk, bow_scene.features_near_words(rng, voc, extra)])
            uv = np.concatenate([uv, np.stack([rng.uniform(0, W, extra), rng.uniform(0, H, extra)], axis=1)])
            lv, ang = np.concatenate([lv, rng.integers(0, NLEVELS, extra)]), np.concatenate([ang, rng.uniform(0, 360, extra)])
            mp, planted = np.concatenate([mp, np.full(extra, -1)]), np.concatenate([planted, np.full(extra, -1)])
        perm = rng.permutation(len(uv))
        finish(s["id"], Tk, uv[perm], lv[perm], ang[perm], dk[perm], mp[perm], planted[perm], s.get("conn", []), s.get("bad", False))

    # ---- the current side: W' = S_d W
    sd = 1.0 if fix_scale else float(scale)
    Sd = pose(rng, 0.4, 3.0)
    Rd, td = Sd[:3, :3], Sd[:3, 3]
    cur_ids = {}
    for pi, pl in enumerate(P):                                        # the current side's own map points: the place seen again
        if pi not in set(sees.values()) | {0}:
            continue
        n = len(pl["ids"])
        Xp = sd * pl["Xw"] @ Rd.T + td + rng.normal(0, pos_noise * sd, (n, 3))
        Tq = pl["Tq"]
        Oq = sd * Rd @ (-Tq[:3, :3].T @ Tq[:3, 3]) + td
        cur_ids[pi] = m.add(Xp, flip(rng, pl["desc"], 0, 4), Oq, pl["level"], origin=pl["ids"])
    truth = {}
    for cid in range(10, max(run) + 1):
        pi = sees.get(cid, 0)
        pl = P[pi]
        n = len(pl["ids"])
        Ti = pose(rng, rng.uniform(0.02, 0.06), 0.15) @ pl["Tq"]                                 # the true pose in W
        Rp = Ti[:3, :3] @ Rd.T
        Tp = np.eye(4)
        Tp[:3, :3], Tp[:3, 3] = Rp, sd * Ti[:3, 3] - Rp @ td                                     # rigid in W'
        S = np.eye(4)
        S[:3, :3], S[:3, 3] = sd * Ti[:3, :3], sd * Ti[:3, 3]
        truth[cid] = S                                                                           # Scw_true = T_iw' S_d
        lv = pl["level"].copy()
        Xp = np.asarray([m.pos[j] for j in cur_ids[pi]])
        uv = project(Tp, Xp)[0] + rng.normal(0, 1, (n, 2)) * (noise * SF[lv])[:, None]
        dk = pl["desc"].copy()
        for g, (lo, hi) in FLIPS.items():
            sel = np.nonzero(pl["group"] == g)[0]
            dk[sel] = flip(rng, pl["desc"][sel], lo, hi)
        ang = pl["angle"] - 24.0 + rng.uniform(-2, 2, n)
        see = rng.random(n) < (0.4 if cid == 10 else 0.85)
        mp = np.where(see, cur_ids[pi], -1)
        idx = np.nonzero(see)[0]
        mp[rng.choice(idx, min(len(idx), 3), replace=False)] = -1                                # keypoints without a map point
        planted = pl["ids"][see]
        uv, lv, ang, dk, mp = uv[see], lv[see], ang[see], dk[see], mp[see]
        if cid in foreign:
            dk = None
        nc = nclutter
        uv = np.concatenate([uv, np.stack([rng.uniform(0, W, nc), rng.uniform(0, H, nc)], axis=1)])
        lv, ang = np.concatenate([lv, rng.integers(0, NLEVELS, nc)]), np.concatenate([ang, rng.uniform(0, 360, nc)])
        mp, planted = np.concatenate([mp, np.full(nc, -1)]), np.concatenate([planted, np.full(nc, -1)])
        kfs[cid] = dict(pending=(Tp, uv, lv, ang, dk, mp, planted), conn=list(range(cid - 1, 9, -1)), bad=cid in bad_current)
    for cid in sorted(k for k in kfs if "pending" in kfs[k]):                                    # clutter after every word in use is known
        Tp, uv, lv, ang, dk, mp, planted = kfs[cid]["pending"]
        conn, bad = kfs[cid]["conn"], kfs[cid]["bad"]
        nown = len(uv) - nclutter
        cd = clutter(rng, voc, ov, held, nclutter + (nown if dk is None else 0))
        dk = np.concatenate([cd[nclutter:] if dk is None else dk, cd[:nclutter]])
        perm = rng.permutation(len(uv))
        finish(cid, Tp, uv[perm], lv[perm], ang[perm], dk[perm], mp[perm], planted[perm], conn, bad)
    for j in rng.choice(np.concatenate(list(cur_ids.values())), 3, replace=False):               # bad points on the current side too
        m.bad[j] = True
    nwords = int((voc["is_leaf"] == 1).sum())
    return dict(seed=seed, voc=voc, nwords=nwords, map=m.freeze(), kfs=kfs, run=list(run), last_loop=int(last_loop), fix_scale=bool(fix_scale),
                Scw_true=truth, scale=sd)


def M(groups=("near", "wide"), **kw):
    return dict(dict(id=3, kind="true", holds=("near", "wide"), groups=groups, conn=[2, 4]), **kw)


def N(kid, **kw):
    """a neighbour of the matched keyframe: it alone sees `far`"""
    return dict(dict(id=kid, kind="true", holds=("far",), groups=("far",), conn=[3, 6 - kid], extra=30, null=1, bad_points=1), **kw)


def OTHER(kid):
    return dict(id=kid, kind="other")


BASE = dict(near=60, wide=40, far=50)
RUN = [12, 13, 14, 15]
# name -> (seed, constructor)
SCENES = {
    "closed": (1, lambda s: make(s, [BASE], [OTHER(0), OTHER(1), N(2), M(), N(4), OTHER(5)], RUN)),
    "too_recent": (1, lambda s: make(s, [BASE], [OTHER(0), OTHER(1), N(2), M(), N(4), OTHER(5)], RUN, last_loop=4)),
    "no_candidates": (1, lambda s: make(s, [BASE], [OTHER(0), OTHER(1), N(2), M(), N(4), OTHER(5)], [12, 13, 14, 15, 16, 17], foreign=(13,))),
    "inconsistent": (1, lambda s: make(s, [BASE, dict(near=60, wide=20)],
                                       [OTHER(0), dict(id=1, kind="true", place=1, conn=[]), N(2), M(), N(4), OTHER(5)], RUN, sees={13: 1, 15: 1})),
    "few_bow": (1, lambda s: make(s, [BASE], [dict(id=0, kind="true", holds=("near", "wide"), keep=0.12, conn=[]),
                                              dict(id=1, kind="true", holds=("near", "wide"), bad=True, conn=[]), N(2), M(), N(4), OTHER(5)], RUN, bad_current=(11,))),
    "decoy_first": (1, lambda s: make(s, [BASE], [dict(id=0, kind="decoy", holds=("near", "wide"), groups=("near",), keep=0.55, conn=[]), OTHER(1), N(2),
                                                  M(kind="copy", pos_noise=0.004, junk=0.5), N(4), OTHER(5)], RUN)),
    "weak_refine": (7, lambda s: make(s, [dict(near=60, wide=30, far=50, bias=60)],
                                      [dict(id=0, kind="copy", holds=("near", "bias"), groups=("near", "bias"), keep=0.6, pos_noise=0.004, bias=7.0, conn=[]),
                                       OTHER(1), N(2), M(holds=("near", "wide", "far")), N(4), OTHER(5)], RUN)),
    "few_total": (1, lambda s: make(s, [dict(near=42, wide=5, far=5)], [OTHER(0), OTHER(1), N(2), M(), N(4), OTHER(5)], RUN)),
    "fixed_scale": (2, lambda s: make(s, [BASE], [OTHER(0), OTHER(1), N(2), M(), N(4), OTHER(5)], RUN, fix_scale=True)),
}
# seeds 1..12 looked at on the CPU chain per scene -> (tried, reached the branch, of those met every condition of the device comparison,
# kept).  The seeds dropped by a condition (closed 7, no_candidates 4, few_bow 12, fixed_scale 7) fuse or match one point that is not the
# planted one: a clutter keypoint whose random descriptor lies within TH_LOW of a loop point's.  decoy_first needs the decoy answered before
# the matched keyframe AND the winner's first hit after pass 0; weak_refine needs the biased copy answered first (3 of 12: 7, 8, 12).
SEEDS_TRIED = {"closed": (12, 12, 11, 1), "too_recent": (12, 12, 12, 1), "no_candidates": (12, 12, 11, 1), "inconsistent": (12, 12, 12, 1),
               "few_bow": (12, 12, 11, 1), "decoy_first": (12, 1, 1, 1), "weak_refine": (12, 3, 3, 7), "few_total": (12, 9, 9, 1),
               "fixed_scale": (12, 12, 11, 2)}


def scene(name, seed=None):
    key = (name, seed)
    if key not in _cache:
        s0, f = SCENES[name]
        sc = f(s0 if seed is None else seed)
        sc["name"] = name
        _cache[key] = sc
    return _cache[key]
