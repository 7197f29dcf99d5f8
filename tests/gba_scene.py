"""Seeded scenes for the bundle adjustment of a loop-closure-sized map (orbb_global_bundle_adjustment, the blocked reduced-system
path of csrc/orbx_lba.hip): lba_scene's camera and noise, but the keyframes stand along x at 2 m steps looking down +z and the points
(4 to 20 m deep) are spread along the whole path, so that a keyframe sees a window of the map and the reduced system has blocks that
are structurally zero.  The last `nloop` keyframes are placed back at the start and see the first points: the loop's blocks, far
from the diagonal.  Only keyframe 0 is fixed, half the observations are stereo, a point with fewer than two observations is dropped."""
import os
import re

import numpy as np

import lba_ref as R
import lba_scene as LS

STEP = 2.0


def _source():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb_slam2v2-1_amd", "csrc", "orbx_lba.hip")).read()


def panel_poses():
    """GBA_PANEL_POSES of csrc/orbx_lba.hip: the poses of one panel of the blocked LDL^T"""
    return int(re.search(r"^#define\s+GBA_PANEL_POSES\s+(\d+)\b", _source(), flags=re.M).group(1))


def tile_edge():
    """GBA_TILE of csrc/orbx_lba.hip: the edge of a tile of the trailing update"""
    return int(re.search(r"^#define\s+GBA_TILE\s+(\d+)\b", _source(), flags=re.M).group(1))


def make(seed, nkf, npts, nloop=0, noise=0.7, rot=0.01, trans=0.05, ptnoise=0.08, lone_pair=None):
    """-> dict(kfs, pts, obs, true_poses [K, 4, 4], true_pts [P, 3], special).  nkf keyframes in all, keyframe 0 fixed; the last
    nloop stand back at the start, between the first keyframes.  lone_pair (a, b): one more point, 60 m deep and midway between
    keyframes a and b, observed by exactly those two - which stand too far apart to share any other point, so their block of the
    reduced system has exactly one contribution."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = LS.CAM
    K = nkf
    xs = STEP * np.arange(K, dtype=np.float64)
    if nloop:
        xs[K - nloop:] = STEP * (np.arange(nloop) + 0.5)
    Ts = []
    for i in range(K):
        Twc = np.eye(4)
        Twc[:3, :3] = LS.rodrigues([0.0, rng.normal(0, 0.01), 0.0])
        Twc[:3, 3] = [xs[i] + rng.normal(0, 0.05), rng.normal(0, 0.05), rng.normal(0, 0.05)]
        Ts.append(np.linalg.inv(Twc))
    Ts = np.array(Ts)
    span = STEP * (K - nloop - 1)
    z = rng.uniform(4.0, 20.0, npts)
    Xw = np.stack([rng.uniform(-3.0, span + 3.0, npts), rng.uniform(-0.12, 0.12, npts) * z, z], 1)
    Xw = Xw[np.argsort(Xw[:, 0], kind="stable")]      # the first points are the ones at the start of the path
    special = {}
    if lone_pair is not None:
        a, b = lone_pair
        special["lone_pair"] = (a, b)
        special["lone_point"] = len(Xw)
        Xw = np.concatenate([Xw, [[0.5 * (xs[a] + xs[b]), 0.3, 60.0]]])
    P = len(Xw)
    obs = []
    for p in range(P):
        Xc = Ts[:, :3, :3] @ Xw[p] + Ts[:, :3, 3]
        u, v = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
        who = np.nonzero((Xc[:, 2] > 0.5) & (u > 0) & (u < LS.W) & (v > 0) & (v < LS.H))[0]
        if p == special.get("lone_point"):
            who = np.array(sorted(lone_pair))
        for k in who:
            oc = int(rng.integers(0, LS.NLEVELS))
            is_st = rng.random() < 0.5
            du, dv = rng.normal(0, noise * LS.SF[oc], 2)
            uu, vv = u[k] + du, v[k] + dv
            ur = uu - bf / Xc[k, 2] + rng.normal(0, noise * LS.SF[oc]) if is_st else -1.0
            if ur < 0:
                ur = -1.0
            obs.append((k, p, uu, vv, ur, LS.INV_SIGMA2[oc]))
    obs = np.array(obs, R.OBS_DTYPE)
    keep = np.bincount(obs["pt"], minlength=P) >= 2      # a point with fewer than two observations is no part of the map
    renum = np.cumsum(keep) - 1
    obs = obs[keep[obs["pt"]]]
    obs["pt"] = renum[obs["pt"]]
    if "lone_point" in special:
        assert keep[special["lone_point"]]
        special["lone_point"] = int(renum[special["lone_point"]])
    Xw = Xw[keep]
    kfs = np.zeros(K, R.KF_DTYPE)
    for i in range(K):
        T = Ts[i].copy()
        if i > 0:
            d = np.eye(4)
            d[:3, :3] = LS.rodrigues(rng.normal(0, rot, 3))
            d[:3, 3] = rng.normal(0, trans, 3)
            T = d @ T
        kfs["Tcw"][i] = T.astype(np.float32).reshape(-1)
        kfs["fixed"][i] = 1 if i == 0 else 0
    kfs["fx"], kfs["fy"], kfs["cx"], kfs["cy"], kfs["bf"] = fx, fy, cx, cy, bf
    pts = np.zeros(len(Xw), R.PT_DTYPE)
    X0 = Xw + rng.normal(0, ptnoise, Xw.shape)
    pts["x"], pts["y"], pts["z"] = X0[:, 0], X0[:, 1], X0[:, 2]
    return dict(kfs=kfs, pts=pts, obs=obs, true_poses=Ts, true_pts=Xw, special=special)


G = panel_poses()
# name -> make() arguments.  The free poses are nkf - 1 (keyframe 0 is fixed): one partial panel, exactly one panel, two panels and a
# remainder (the trailing update runs twice); window_loop: 40 free poses with structurally zero blocks and the loop's blocks;
# crowded: the same path with so many points that a keyframe has more observations than the 256 threads that own a block's sum,
# and one block with exactly one contribution (keyframes 5 and 30 stand 50 m apart and share the lone point only).
CASES = {
    "one_short": dict(seed=701, nkf=G, npts=90),
    "one_panel": dict(seed=702, nkf=G + 1, npts=100),
    "two_and_rest": dict(seed=703, nkf=2 * G + 4, npts=220),
    "window_loop": dict(seed=704, nkf=41, npts=420, nloop=4),
    "crowded": dict(seed=705, nkf=41, npts=1500, nloop=4, lone_pair=(5, 30)),
}
ITERATIONS = 10
_cache, _refs = {}, {}


def schedule():
    """LoopClosing::RunGlobalBundleAdjustment's call: GlobalBundleAdjustemnt(mpMap, 10, &mbStopGBA, nLoopKF, false)"""
    return R.schedule_global(ITERATIONS, False)


def case(name):
    if name not in _cache:
        _cache[name] = make(**CASES[name])
    return _cache[name]


def pattern(sc, active=None):
    """-> (blocks, contributions, pairs): a numpy enumeration of the column pairs (i1 <= i2) that share an active point, for the
    round whose active edges are given (all of them by default); pairs is the set of (i1, i2)"""
    o = sc["obs"]
    act = np.ones(len(o), bool) if active is None else active
    free = sc["kfs"]["fixed"] == 0
    has = np.zeros(len(sc["kfs"]), bool)
    has[o["kf"][act]] = True
    col = np.cumsum(free & has) - 1
    col[~(free & has)] = -1
    sel = act & (col[o["kf"]] >= 0)
    M = np.zeros((int(col.max()) + 1 if len(col) else 0, len(sc["pts"])), np.int64)
    M[col[o["kf"][sel]], o["pt"][sel]] = 1
    C = M @ M.T      # C[i1, i2]: the points both columns observe
    iu = np.triu_indices(len(C))
    return int((C[iu] > 0).sum()), int(C[iu].sum()), {(int(a), int(b)) for a, b in zip(*iu) if C[a, b] > 0}


def reference(name):
    """as lba_scene.reference under the global schedule: (scene, the restatement's result, its DRAWS draws, S)"""
    if name not in _refs:
        sc = case(name)
        ref = R.optimize(sc["kfs"], sc["pts"], sc["obs"], schedule=schedule())
        rng = np.random.default_rng(4321)
        draws = [R.optimize(sc["kfs"], sc["pts"], sc["obs"], schedule=schedule(), order=rng, perturb=rng) for _ in range(LS.DRAWS)]
        dev = max([0.0] + [float(np.abs(LS.estimates(d) - LS.estimates(ref)).max()) for d in draws])
        _refs[name] = (sc, ref, draws, dev)
    return _refs[name]
