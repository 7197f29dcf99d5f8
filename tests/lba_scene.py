"""Seeded Optimizer::LocalBundleAdjustment scenes: keyframes on a slightly curved path looking down +z, map points 4 to 20 m in front
of them, every point observed by the keyframes that see it (at least two), keypoints with pixel noise scaled by the level sigma,
a stated fraction of gross outliers; the poses of the free keyframes and all points start next to the truth."""
import os
import re

import numpy as np

import lba_ref as R

NLEVELS, SCALE = 8, 1.2
SF = (np.float32(SCALE) ** np.arange(NLEVELS)).astype(np.float32)
INV_SIGMA2 = (np.float32(1.0) / (SF * SF)).astype(np.float32)
CAM = (718.856, 718.856, 607.19, 185.2, 386.1448)       # fx fy cx cy bf: KITTI-00
W, H = 1241, 376
MARGIN = 1e-5       # |chi2 / threshold - 1| and |depth| below which a flag may differ; the value tests/test_poseopt_gpu.py uses
DRAWS = 16
GRAZE_X = 40.0     # metres to the side of keyframe 0, in its image plane: in front of the last keyframes, which are turned towards it


def lds_poses():
    """LBA_LDS_POSES of csrc/orbx_lba.hip: the free poses whose reduced system is factorised in LDS"""
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb_slam2v2-1_amd", "csrc", "orbx_lba.hip")).read()
    return int(re.search(r"^#define\s+LBA_LDS_POSES\s+(\d+)\b", txt, flags=re.M).group(1))


def rodrigues(rvec):
    rvec = np.asarray(rvec, np.float64)
    th = np.linalg.norm(rvec)
    K = np.array([[0, -rvec[2], rvec[1]], [rvec[2], 0, -rvec[0]], [-rvec[1], rvec[0], 0]])
    return np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def make(seed, nfree, nfixed, npts, stereo=0.0, outliers=0.0, noise=0.7, rot=0.01, trans=0.05, ptnoise=0.08, first_id0=False,
         behind=False, grazing=False, dead_point=False, dead_pose=False, shuffle=False, idle=0, turned=False, plane_point=False):
    """-> dict(kfs, pts, obs, true_poses [K, 4, 4], true_pts [P, 3], gross [E] bool, special: names -> indices).
    stereo: the fraction of stereo observations (0: monocular only, 1: stereo only).  first_id0: the first local keyframe is fixed
    (mnId == 0).  behind: one more point BEHIND keyframe 0, observed by keyframes 0 and 1.  grazing: one more point in the image plane
    of keyframe 0 (depth 0 at the truth), seen by it with inv_sigma2 = 0 (chi2 = 0: only the depth test can flag it) and by two others.
    dead_point: one more point whose observations are all gross outliers.  dead_pose: one more free keyframe whose observations are
    all gross outliers.  shuffle: the observations in a random order.  idle: that many fixed keyframes without any observation IN FRONT of
    the others, so that the keyframes that matter lie past the first workgroup of a kernel that takes one keyframe per thread.
    turned: three keyframes around the points whose Tcw are rotations of 3 rad about x, y and z - a negative trace with each diagonal
    entry the largest once, where the path's keyframes (a few hundredths of a radian) all have a positive one.
    plane_point: the first fixed keyframe's Tcw is the identity, and the first point it observes starts with z == 0.0 exactly: that
    edge's depth is an exact zero, 1 / z is infinite, and every linearisation of round 1 holds non-finite entries."""
    rng = np.random.default_rng(seed)
    K = nfree + nfixed
    fx, fy, cx, cy, bf = CAM
    Ts = []
    for i in range(K):          # the free (local) keyframes first, as the reference adds them
        Twc = np.eye(4)
        Twc[:3, :3] = rodrigues([0.0, 0.03 * i + rng.normal(0, 0.01), 0.0])
        Twc[:3, 3] = [0.6 * i + rng.normal(0, 0.05), rng.normal(0, 0.05), 0.25 * i]
        Ts.append(np.linalg.inv(Twc))
    Ts = np.array(Ts)
    if plane_point:
        assert nfixed > 0
        Ts[nfree] = np.eye(4)
    z = rng.uniform(4.0, 20.0, npts)
    Xw = np.stack([rng.uniform(-0.45, 0.45, npts) * z + 0.3 * K, rng.uniform(-0.12, 0.12, npts) * z, z + 0.1 * K], 1)
    if turned:      # Rcw = 3 rad about x, y, z; every keyframe 16 m from the middle of the points, which lie closer together, looking at it
        assert K == 3
        mid = np.array([0.3 * K, 0.0, 12.0 + 0.1 * K])
        Xw = mid + (Xw - mid) * [0.35, 0.5, 1.0]
        for i in range(K):
            Ts[i] = np.eye(4)
            Ts[i, :3, :3] = rodrigues(3.0 * np.eye(3)[i])
            Ts[i, :3, 3] = -Ts[i, :3, :3] @ (mid - 16.0 * Ts[i, 2, :3])      # the optical axis in the world is the third row of Rcw
    special = {}
    extra = []
    if behind:
        special["behind"] = len(Xw) + len(extra); extra.append(np.linalg.inv(Ts[0])[:3, :3] @ np.array([0.4, 0.1, -3.0]) + np.linalg.inv(Ts[0])[:3, 3])
    if grazing:
        special["grazing"] = len(Xw) + len(extra); extra.append(np.linalg.inv(Ts[0])[:3, :3] @ np.array([GRAZE_X, 0.2, 0.0]) + np.linalg.inv(Ts[0])[:3, 3])
    if dead_point:
        special["dead_point"] = len(Xw) + len(extra); extra.append(np.array([0.3 * K, 0.1, 9.0]))
    if extra:
        Xw = np.concatenate([Xw, np.array(extra)])
    P = len(Xw)
    kfs = np.zeros(K + (1 if dead_pose else 0), R.KF_DTYPE)
    if dead_pose:
        Twc = np.eye(4)
        Twc[:3, 3] = [0.6 * K, 0.0, 0.25 * K]
        Ts = np.concatenate([Ts, np.linalg.inv(Twc)[None]])
        special["dead_pose"] = K
    Kall = len(Ts)
    obs, gross = [], []
    for p in range(P):
        Xc = Ts[:, :3, :3] @ Xw[p] + Ts[:, :3, 3]
        with np.errstate(all="ignore"):
            u, v = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
        vis = (Xc[:, 2] > 0.5) & (u > 0) & (u < W) & (v > 0) & (v < H)
        who = np.nonzero(vis)[0]
        if p == special.get("behind"):
            who = np.array([0, 1])
        elif p == special.get("grazing"):
            front = np.nonzero(Xc[:, 2] > 0.3)[0]
            who = np.concatenate([[0], front[front != 0][-2:]])      # in front of the last keyframes, wherever it projects
        elif len(who) > 1 and rng.random() < 0.3:
            who = rng.permutation(who)[:max(2, len(who) // 2)]
        if dead_pose:
            who = who[who != K]
        for k in np.sort(who):
            oc = int(rng.integers(0, NLEVELS))
            is_st = rng.random() < stereo
            g = rng.random() < outliers or p == special.get("dead_point")
            du, dv = rng.normal(0, noise * SF[oc], 2)
            if g:
                du, dv = rng.choice([-1, 1], 2) * rng.uniform(20, 90, 2)
            uu, vv = u[k] + du, v[k] + dv
            ur = uu - bf / Xc[k, 2] + rng.normal(0, noise * SF[oc]) if is_st and Xc[k, 2] > 0.5 else -1.0
            if is_st and ur < 0:      # the right keypoint would lie outside the image: no stereo observation
                if stereo >= 1.0:
                    continue
                ur = -1.0
            is2 = INV_SIGMA2[oc]
            if p == special.get("grazing") and k == 0:
                uu, vv, ur, is2 = cx, cy, -1.0, 0.0
            if not np.isfinite(uu + vv):
                uu, vv = cx, cy
            obs.append((k, p, uu, vv, ur, is2)); gross.append(g)
    if dead_pose:      # ten observations that fit no pose
        for p in rng.permutation(npts)[:10]:
            obs.append((K, p, rng.uniform(0, W), rng.uniform(0, H), -1.0, INV_SIGMA2[0])); gross.append(True)
    obs = np.array(obs, R.OBS_DTYPE)
    gross = np.array(gross)
    if shuffle:
        perm = np.random.default_rng(seed + 7919).permutation(len(obs))      # a generator of its own: the rest of the scene is the unshuffled one
        obs, gross = obs[perm], gross[perm]
    # the start: free poses and all points moved off the truth
    for i in range(Kall):
        T = Ts[i].copy()
        free = i < nfree and not (first_id0 and i == 0) or (dead_pose and i == K)
        if free:
            d = np.eye(4)
            d[:3, :3] = rodrigues(rng.normal(0, rot, 3))
            d[:3, 3] = rng.normal(0, trans, 3)
            T = d @ T
        kfs["Tcw"][i] = T.astype(np.float32).reshape(-1)
        kfs["fixed"][i] = 0 if free else 1
    kfs["fx"], kfs["fy"], kfs["cx"], kfs["cy"], kfs["bf"] = fx, fy, cx, cy, bf
    pts = np.zeros(P, R.PT_DTYPE)
    X0 = Xw + rng.normal(0, ptnoise, Xw.shape)
    pts["x"], pts["y"], pts["z"] = X0[:, 0], X0[:, 1], X0[:, 2]
    if plane_point:
        special["plane_kf"] = nfree
        special["plane_point"] = int(obs["pt"][obs["kf"] == nfree][0])
        pts["z"][special["plane_point"]] = 0.0
    if idle:
        front = np.zeros(idle, R.KF_DTYPE)
        front["Tcw"] = np.eye(4, dtype=np.float32).reshape(-1)
        front["Tcw"][:, 3] = np.arange(idle, dtype=np.float32)
        front["fx"], front["fy"], front["cx"], front["cy"], front["bf"], front["fixed"] = fx, fy, cx, cy, bf, 1
        kfs = np.concatenate([front, kfs])
        obs["kf"] += idle
        Ts = np.concatenate([np.tile(np.eye(4), (idle, 1, 1)), Ts])
    return dict(kfs=kfs, pts=pts, obs=obs, true_poses=Ts, true_pts=Xw, gross=gross, special=special)


L = lds_poses()
# The shapes the tests run, smallest where the kernels can go wrong (more than one workgroup of edges, sizes that are no multiple of
# 256 or 64): name -> make() arguments.  The constants that choose a path: LBA_LDS_POSES (nfL, nfL+1) and the 256 threads of a
# workgroup - observations (every case has more), points (wide: 300) and keyframes (many_kf: 306) on both sides of it.  No kernel
# loops by lane over a point's observations (a point is one thread), so there is no case of a point seen by more than 64 keyframes.
# The Levenberg branches (optimization_algorithm_levenberg.cpp:100-161; tests/test_lm_branches_cpu.py counts them): most cases accept
# every trial; outliers and shuffled reject once and accept (AAAAAAAArA); nf0 rejects in a row without a free pose; far_start rejects
# four times in a row with four free poses and recovers (ArrrrAA, every |rho| > 1e-4); far_outliers rejects in three iterations
# (AAArrArrArrrrrA, its last |rho| 6e-9); plane_point fails every solve of round 1 (tempChi = DBL_MAX, a NaN rho, one trial per
# iteration) and leaves round 1 with every estimate as it came.
CASES = {
    "mono": dict(seed=501, nfree=4, nfixed=2, npts=60),
    "stereo": dict(seed=502, nfree=4, nfixed=2, npts=60, stereo=1.0),
    "mixed": dict(seed=503, nfree=5, nfixed=2, npts=70, stereo=0.5),
    "outliers": dict(seed=504, nfree=5, nfixed=2, npts=90, stereo=0.5, outliers=0.1),
    "behind": dict(seed=505, nfree=4, nfixed=2, npts=50, behind=True),
    "grazing": dict(seed=605, nfree=4, nfixed=2, npts=50, grazing=True, outliers=0.05),
    "dead_point": dict(seed=507, nfree=4, nfixed=2, npts=50, dead_point=True),
    "dead_pose": dict(seed=508, nfree=4, nfixed=2, npts=60, dead_pose=True),
    "id0": dict(seed=509, nfree=4, nfixed=1, npts=50, first_id0=True, stereo=0.5),
    "no_fixed": dict(seed=510, nfree=5, nfixed=0, npts=60, stereo=1.0),
    "nf0": dict(seed=511, nfree=0, nfixed=4, npts=50, stereo=0.5, outliers=0.05),
    "shuffled": dict(seed=504, nfree=5, nfixed=2, npts=90, stereo=0.5, outliers=0.1, shuffle=True),
    "nfL": dict(seed=512, nfree=L, nfixed=2, npts=120, stereo=0.5, outliers=0.05),
    "nfL+1": dict(seed=513, nfree=L + 1, nfixed=2, npts=120, stereo=0.5, outliers=0.05),
    "wide": dict(seed=514, nfree=6, nfixed=2, npts=300, stereo=0.3, outliers=0.05),
    "many_kf": dict(seed=515, nfree=4, nfixed=2, npts=50, stereo=0.5, idle=300),
    "turned": dict(seed=516, nfree=2, nfixed=1, npts=12, stereo=0.5, turned=True),
    "far_start": dict(seed=901, nfree=4, nfixed=2, npts=40, stereo=0.5, rot=0.2, trans=0.8, ptnoise=0.8),
    "far_outliers": dict(seed=905, nfree=4, nfixed=2, npts=40, stereo=0.5, outliers=0.1, rot=1.2, trans=4.0, ptnoise=3.0),
    "plane_point": dict(seed=518, nfree=4, nfixed=2, npts=50, stereo=0.5, rot=0.001, trans=0.005, ptnoise=0.008, plane_point=True),
}
# The cases whose counts are compared in every round whatever min |rho| says: the restatement reports min |rho| = 0 for a NaN rho,
# and plane_point's round 1 is five NaN rhos - a NaN is no rounding noise about zero, both sides must reject on it.
COUNTS_ALWAYS = ("plane_point",)


def depth_exempt(name):
    """-> the edges whose depth is an exact 0.0 by construction (plane_point: a point with z == 0.0 seen by a keyframe whose Tcw is
    the identity): z > 0 on an exact zero is not decided by rounding, so the |depth| > MARGIN condition leaves that one edge out"""
    sc = case(name)
    if "plane_point" not in sc["special"]:
        return np.zeros(len(sc["obs"]), bool)
    return (sc["obs"]["kf"] == sc["special"]["plane_kf"]) & (sc["obs"]["pt"] == sc["special"]["plane_point"])
_cache, _refs = {}, {}


def initial_map(seed=520, npts=80):
    """what CreateInitialMapMonocular hands to GlobalBundleAdjustemnt(mpMap, 20): two keyframes, the first with mnId == 0 (fixed),
    monocular observations of every point in both"""
    sc = make(seed=seed, nfree=2, nfixed=0, npts=npts, first_id0=True, trans=0.02)
    both = np.bincount(sc["obs"]["pt"], minlength=len(sc["pts"]))[sc["obs"]["pt"]] == 2
    sc["obs"] = sc["obs"][both]
    return sc


def case(name):
    if name not in _cache:
        _cache[name] = make(**CASES[name])
    return _cache[name]


def estimates(res):
    return np.concatenate([res["kf_est"].reshape(-1), res["pt_est"].reshape(-1)])


def reference(name):
    """-> (scene, the restatement's result, its DRAWS results with every sum in a random order and every sin / cos moved by up to +-2
    ulp, S: its largest deviation in the double estimates over those).  Computed once, shared by the CPU and the GPU tests."""
    if name not in _refs:
        sc = case(name)
        ref = R.optimize(sc["kfs"], sc["pts"], sc["obs"])
        rng = np.random.default_rng(4321)
        draws = [R.optimize(sc["kfs"], sc["pts"], sc["obs"], order=rng, perturb=rng) for _ in range(DRAWS)]
        dev = max([0.0] + [float(np.abs(estimates(d) - estimates(ref)).max()) for d in draws])
        _refs[name] = (sc, ref, draws, dev)
    return _refs[name]
