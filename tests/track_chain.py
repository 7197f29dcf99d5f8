"""Tracking::Track's main loop chained over the synthetic sequences of tests/track_scene.py with NOTHING planted after the first
pose: every matcher projects with a pose the chain estimated itself, and where the reference calls Optimizer::PoseOptimization the
chain calls the library's pose solver on what the matchers just gave it.  (tests/tracking_chain.py, which bench.py times, projects
with the sequence's true pose and applies a chi2 test there instead.)

STEREO, per frame (line numbers: src/Tracking.cc):
    Frame(stereo): extract L / R, ComputeStereoMatches                                       src/Frame.cc:61-120, 481-655
    t = 0  StereoInitialization: the planted first pose, a map point per keypoint with depth  :652-704
    t > 0  TrackWithMotionModel                                                               :1010-1071
             UpdateLastFrame: temporal points by depth order (localization mode)              :944-1008
             pose = mVelocity * mLastFrame.mTcw (an empty velocity: the last pose)            :1018
             SearchByProjection(cur, last, 7; 14 below 20 matches); below 20: lost            :1028-1038
             PoseOptimization                                                                 :1041
             an outlier loses its point, its flag is reset, the point gets mbTrackInView = false and mnLastFrameSeen = this
             frame, so that SearchLocalPoints steps over it; nmatchesMap counts Observations() > 0; below 10: lost   :1044-1070
           TrackLocalMap                                                                      :1073-1117
             SearchLocalPoints: a held point is marked seen; isInFrustum(0.5) over the local points not seen in this frame;
             SearchByProjection(cur, local points, 1) with ORBmatcher(0.8)                    :1288-1338
             PoseOptimization                                                                 :1083
             mnMatchesInliers counts the inliers with Observations() > 0 (the rule of the mapping mode: the stricter of the two);
             STEREO: an outlier loses its point here (its flag stays set: stale, src/Optimizer.cc:286-288 resets only entries with
             a point); MONOCULAR: it keeps it until the sweep at the end of Track(); below 30: lost   :1084-1116
           mVelocity = mTcw * LastTwc, LastTwc from GetRotationInverse / GetCameraCenter      :566-571
           every 4th frame a key frame, then the temporal points are cleaned (in the order of tests/tracking_chain.py);
           new points are placed with the ESTIMATED pose                                      :578-600, 1206-1286
           outliers that still hold a point lose it                                           :606-610
    The local map is every map point that is not temporal, as in tests/tracking_chain.py; the last frame keeps the pose it was
    given (UpdateLastFrame's Tlr * pRef->GetPose() is that pose: nothing moves a key frame here).

MONOCULAR, on the left images:
    MonocularInitialization on frames 0 and 1 (2 x nFeatures extractor)                       :706-778
        mvbPrevMatched = the first frame's keypoints; ORBmatcher(0.9, true).SearchForInitialization(.., 100); below 100: refused
        Initializer(frame, 1.0, 200)::Initialize, its eight-point sets drawn ONCE from a generator seeded by the scene: the same
        for every backend; a match that was not triangulated is dropped
    CreateInitialMapMonocular                                                                 :780-880
        a map point per match; ComputeDistinctiveDescriptors over its two observations (src/MapPoint.cc:252-317);
        UpdateNormalAndDepth with the current key frame as reference (src/MapPoint.cc:340-383); the first key frame's median depth
        (src/KeyFrame.cc:636-666) set to 1: the baseline and the points are scaled - and, as in the reference, the distance ranges
        are NOT (SetWorldPos moves the point only); medianDepth < 0 or fewer than 100 tracked points: reset
        OMITTED: Optimizer::GlobalBundleAdjustemnt (:829) - the library has no bundle adjustment.
    the following frames (nFeatures extractor): TrackWithMotionModel with th 15 and bMono, TrackLocalMap with monocular edges
    (ur = -1), the velocity; no local mapper: no point is ever added.  Chain.recompute_ranges() is the one piece of the mapper a
    scene may call between two frames (tests/track_scene.py says where and why); the tracking code itself never does.
    ONE DEVIATION: the first frame after the initialisation takes the motion model with the initialisation's relative pose as its
    velocity, where the reference takes TrackReferenceKeyFrame (the velocity is empty there).  The scene moves in uniform steps, so
    this is the right prediction; SearchByBoW is chained in tests/reloc_chain.py and tests/loop_chain.py.

TWO RULES OF THE RELOCALISATION WINDOW ARE NOT APPLIED, in both chains, as in tests/tracking_chain.py: mnLastRelocFrameId starts at 0,
so in the reference every frame of these short sequences still counts as "recently relocalised":
    :1110  mnMatchesInliers < 50 while mnId < mnLastRelocFrameId + mMaxFrames: the chain applies the rule that holds afterwards, 30
           (the monocular frames, 59 and 38 inliers, would be lost or near lost under 50);
    :1334  SearchLocalPoints with th = 5 while mnId < mnLastRelocFrameId + 2 (the stereo frame 1): the chain searches with th = 1.

cv::Mat products of float matrices (the prediction, the velocity, the camera centre) accumulate in double and round once, as
cv::gemm does for small CV_32F matrices.

TEST INFRASTRUCTURE.  The bookkeeping above is host code identical for every backend; a backend supplies the device operations
(frame, SearchByProjection(cur, last), SearchLocalPoints, PoseOptimization, SearchForInitialization, Initialize,
ComputeDistinctiveDescriptors).  Every stage call leaves a trace entry: dict(stage, frame, in, out).

MUTATIONS names deliberately wrong versions of the bookkeeping (Chain(..., mutate=name)); they exist so that the scenes can be shown
to notice each join between two stages and are never used by a test that compares backends."""
import numpy as np

import tracking_chain as TC

PKG = TC.PKG
FX, FY, CX, CY, BF = TC.FX, TC.FY, TC.CX, TC.CY, TC.BF
NLEVELS, SCALE = TC.NLEVELS, TC.SCALE
K4 = (FX, FY, CX, CY)
CAM = (FX, FY, CX, CY, BF, float(np.float32(BF) / np.float32(FX)))
MUTATIONS = ("sigma2_of_level_0", "keep_outliers_before_local_search", "velocity_transposed", "stereo_edges_without_ur",
             "mono_outliers_nulled_in_local_map")


class Lost(Exception):
    """a rule of the reference ended the tracking: (frame, rule, count)"""


def mul(a, b):
    """cv::Mat a * b for CV_32F"""
    return (np.asarray(a, np.float64) @ np.asarray(b, np.float64)).astype(np.float32)


def twc_of(Tcw):
    """Frame::UpdatePoseMatrices (src/Frame.cc:261-268): mRwc = mRcw.t(), mOw = -mRcw.t() * mtcw, as the 4x4 LastTwc of :568-570"""
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = Tcw[:3, :3].T
    T[:3, 3] = -mul(Tcw[:3, :3].T, Tcw[:3, 3])
    return T


def init_sets(seed, n, iterations=200):
    """mvSets of Initializer::Initialize (src/Initializer.cc:78-97) from a generator seeded by the scene"""
    import init_ref
    rng = np.random.default_rng([int(seed), 8])
    return init_ref.draw_sets(n, iterations, lambda lo, hi: int(rng.integers(lo, hi + 1)))


class Chain:
    def __init__(self, backend, mode, seed=0, mutate=None):
        assert mode in ("stereo", "mono") and (mutate is None or mutate in MUTATIONS)
        self.be, self.mode, self.mono, self.seed, self.mutate = backend, mode, mode == "mono", seed, mutate
        self.mb = CAM[5]
        self.th_depth = float(np.float32(BF) * np.float32(TC.TH_DEPTH) / np.float32(FX))
        sf = [np.float32(1.0)]
        for _ in range(NLEVELS - 1):
            sf.append(np.float32(sf[-1] * np.float64(np.float32(SCALE))))     # mvScaleFactor (src/ORBextractor.cc:415-420)
        self.sf = np.array(sf, np.float32)
        self.inv_sigma2 = (np.float32(1.0) / (self.sf * self.sf)).astype(np.float32)       # mvInvLevelSigma2 (:421-430)
        self.log_sf = float(np.log(np.float32(SCALE)).astype(np.float32))
        self.map = TC.MapStore()
        self.last, self.vel, self.t = None, None, 0
        self.trace, self.frames, self.poses = [], [], []      # stage calls; per tracked frame the counts; per frame the pose
        self.init = None

    def _log(self, stage, inp, out):
        self.trace.append(dict(stage=stage, frame=self.t, **{"in": inp}, out=out))

    # ---- the state a second chain continues from (the last frame's device handle is rebuilt by extracting it again)
    def state(self):
        import copy
        L = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.last.items() if k != "frame"}
        return dict(map=copy.deepcopy(self.map), last=L, vel=None if self.vel is None else self.vel.copy(), t=self.t)

    def restore(self, st, last_images):
        """stereo: continue from state(); last_images = the (left, right) of the last frame"""
        import copy
        self.map, self.vel, self.t = copy.deepcopy(st["map"]), None if st["vel"] is None else st["vel"].copy(), st["t"]
        self.last = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st["last"].items()}
        f = self.be.frame_stereo(*last_images)
        assert f["k"].tobytes() == self.last["k"].tobytes() and f["d"].tobytes() == self.last["d"].tobytes()
        self.last["frame"] = f

    # ---- geometry (host code, float32 like Frame::UnprojectStereo, src/Frame.cc:657-672)
    def _unproject(self, k, depth, Twc):
        z = depth.astype(np.float32)
        x = ((k["x"] - np.float32(CX)) * z * np.float32(1.0 / FX)).astype(np.float32)
        y = ((k["y"] - np.float32(CY)) * z * np.float32(1.0 / FY)).astype(np.float32)
        pc = np.stack([x, y, z], 1)
        return (pc @ Twc[:3, :3].T + Twc[:3, 3]).astype(np.float32)

    def _ranges(self, pos, ow, lvl):
        """distance, unit direction and the range of MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:369-379) seen from ow"""
        po = (pos - ow).astype(np.float32)
        dist = np.sqrt((po.astype(np.float64) ** 2).sum(1)).astype(np.float32)
        unit = (po / np.maximum(dist, np.float32(1e-12))[:, None]).astype(np.float32)
        maxd = (dist * self.sf[lvl]).astype(np.float32)
        return unit, maxd, (maxd / self.sf[NLEVELS - 1]).astype(np.float32)

    def _new_points(self, k, d, depth, idx, Twc, obs, temporal):
        pos = self._unproject(k[idx], depth[idx], Twc)
        normal, maxd, mind = self._ranges(pos, Twc[:3, 3].astype(np.float32), k["octave"][idx])
        return self.map.add(pos, d[idx], normal, maxd, mind, obs, temporal)

    def _close_points_order(self, depth, has_point):
        """the indices UpdateLastFrame / CreateNewKeyFrame visit (:957-1007 and the same loop of CreateNewKeyFrame) that need a new point"""
        idx = np.nonzero(depth > 0)[0]
        order = idx[np.lexsort((idx, depth[idx]))]          # sort(pair<float,int>): depth, then index
        create, npts = [], 0
        for i in order:
            if not has_point[i]:
                create.append(i)
            npts += 1
            if depth[i] > self.th_depth and npts > 100:
                break
        return np.array(create, np.int64)

    # ---- Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:239-453): what it reads of the frame
    def _optimize(self, stage, f, mp, Tcw, outlier):
        m, k = self.map, f["k"]
        import pose_ref
        has = mp >= 0
        p = m.pos[np.maximum(mp, 0)] if len(m.pos) else np.zeros((len(mp), 3), np.float32)
        obs = np.zeros(len(mp), pose_ref.OBS_DTYPE)
        is2 = self.inv_sigma2 if self.mutate != "sigma2_of_level_0" else np.full(NLEVELS, self.inv_sigma2[0], np.float32)
        ur = f["uright"] if self.mutate != "stereo_edges_without_ur" else np.full(len(k), -1.0, np.float32)
        obs["valid"], obs["u"], obs["v"], obs["ur"], obs["inv_sigma2"] = has, k["x"], k["y"], ur, is2[k["octave"]]
        for j, a in enumerate(("wx", "wy", "wz")):
            obs[a] = np.where(has, p[:, j], 0)
        T, out, ngood, info = self.be.optimize(f, obs, is2, Tcw, outlier)
        self._log(stage, dict(obs=obs, Tcw=Tcw.copy(), outlier=outlier.copy()), dict(Tcw=T, outlier=out, ngood=ngood, info=info))
        if int(has.sum()) < 3:                                            # :364-365 returns before SetPose
            return Tcw.copy(), np.asarray(out, np.uint8).copy(), int(ngood)
        return np.asarray(T, np.float32).copy(), np.asarray(out, np.uint8).copy(), int(ngood)

    # ---- the part of Track() every frame after the first shares
    def _track(self, f):
        be, m, L, mono, mut = self.be, self.map, self.last, self.mono, self.mutate
        k, n = f["k"], len(f["k"])
        c = dict(frame=self.t)
        if not mono:
            # UpdateLastFrame: temporal points (Observations() == 0) for the close stereo keypoints of the last frame
            has = (L["mp"] >= 0) & (m.obs[np.maximum(L["mp"], 0)] >= 1)
            cr = self._close_points_order(L["depth"], has)
            if len(cr):
                L["mp"][cr] = self._new_points(L["k"], L["d"], L["depth"], cr, L["Twc"], 0, True)
        Tpred = L["Tcw"].copy() if self.vel is None else mul(self.vel, L["Tcw"])
        self._log("predict", dict(velocity=None if self.vel is None else self.vel.copy(), last=L["Tcw"].copy()), dict(Tcw=Tpred))
        lp = np.zeros(len(L["k"]), be.LASTPT_DTYPE)
        hm = L["mp"] >= 0
        ids = np.maximum(L["mp"], 0)
        lp["has_mp"] = hm
        lp["wx"], lp["wy"], lp["wz"] = m.pos[ids, 0], m.pos[ids, 1], m.pos[ids, 2]
        lp["observations"] = np.where(hm, m.obs[ids], 0)
        lp["octave"], lp["angle"] = L["k"]["octave"], L["k"]["angle"]
        th = 15.0 if mono else 7.0                                            # :1023-1027
        for th_ in (th, 2 * th):
            nm, cur = be.search_frame(f, L["frame"], Tpred, L["Tcw"], lp, np.full(n, -1, np.int32), th_, mono)
            self._log("project", dict(Tcw=Tpred.copy(), last_Tcw=L["Tcw"].copy(), last=lp, last_desc=L["d"], th=th_, mono=mono), dict(n=nm, match=cur))
            if nm >= 20:
                break
        c["proj"] = int(nm)
        if nm < 20:
            raise Lost(self.t, "projection matches < 20", nm)
        mp = np.full(n, -1, np.int64)
        got = cur >= 0
        mp[got] = L["mp"][cur[got]]
        outlier = np.zeros(n, np.uint8)                                      # Frame's constructor: mvbOutlier(N, false)
        Tcw, outlier, _ = self._optimize("optimize_motion", f, mp, Tpred, outlier)
        # :1044-1062
        seen = np.zeros(len(m.obs), bool)                                    # mnLastFrameSeen == this frame
        o1 = (mp >= 0) & (outlier != 0)
        c["outliers_motion"] = int(o1.sum())
        if mut != "keep_outliers_before_local_search":
            seen[mp[o1]] = True
            mp[o1] = -1
            outlier[o1] = 0
        c["matches_map"] = int(((mp >= 0) & (m.obs[np.maximum(mp, 0)] > 0)).sum())
        self._log("discard", dict(outlier=o1.copy()), dict(mp=mp.copy(), matches_map=c["matches_map"]))
        if c["matches_map"] < 10:
            raise Lost(self.t, "nmatchesMap < 10", c["matches_map"])
        # SearchLocalPoints over the local map (every non-temporal point)
        seen[mp[mp >= 0]] = True
        loc = np.nonzero(m.alive & ~m.temporal)[0]
        pos_in_loc = np.full(len(m.obs), -1, np.int64)
        pos_in_loc[loc] = np.arange(len(loc))
        wp = np.zeros(len(loc), be.WORLDPOINT_DTYPE)
        wp["valid"] = ~seen[loc]
        wp["wx"], wp["wy"], wp["wz"] = m.pos[loc, 0], m.pos[loc, 1], m.pos[loc, 2]
        wp["nx"], wp["ny"], wp["nz"] = m.normal[loc, 0], m.normal[loc, 1], m.normal[loc, 2]
        wp["max_distance"] = (np.float32(1.2) * m.maxd[loc]).astype(np.float32)     # GetMaxDistanceInvariance (src/MapPoint.cc:397-407)
        wp["min_distance"] = (np.float32(0.8) * m.mind[loc]).astype(np.float32)
        wp["observations"] = m.obs[loc]
        pid = np.maximum(mp, 0)
        fm = np.where(mp >= 0, np.where(m.temporal[pid], -2, pos_in_loc[pid]), -1).astype(np.int32)
        ext_obs = np.where(mp >= 0, m.obs[pid], 0).astype(np.int32)
        nm2, fm2, proj = be.search_local(f, wp, m.desc[loc], Tcw, fm, ext_obs, 1.0, 0.8, self.log_sf)
        self._log("local", dict(pts=wp, desc=m.desc[loc], Tcw=Tcw.copy(), holder=fm, ext_obs=ext_obs), dict(n=nm2, holder=fm2, frustum=proj))
        newh = (fm2 >= 0) & (fm2 != fm)
        mp[newh] = loc[fm2[newh]]
        c["local"], c["in_view"] = int(newh.sum()), int((proj["in_view"] != 0).sum())
        Tcw, outlier, _ = self._optimize("optimize_local", f, mp, Tcw, outlier)
        # :1084-1106
        o2 = (mp >= 0) & (outlier != 0)
        c["outliers_local"] = int(o2.sum())
        c["inliers"] = int(((mp >= 0) & ~o2 & (m.obs[np.maximum(mp, 0)] > 0)).sum())
        if not mono or mut == "mono_outliers_nulled_in_local_map":
            mp[o2] = -1
        self._log("track_local_map", dict(outlier=o2.copy()), dict(mp=mp.copy(), inliers=c["inliers"]))
        if c["inliers"] < 30:
            raise Lost(self.t, "mnMatchesInliers < 30", c["inliers"])
        Twc = twc_of(Tcw)
        # :566-571
        self.vel = mul(Tcw, L["Twc"]) if mut != "velocity_transposed" else mul(L["Twc"], Tcw)
        self._log("velocity", dict(Tcw=Tcw.copy(), last_Twc=L["Twc"].copy()), dict(velocity=self.vel.copy()))
        if not mono:
            depth, d = f["depth"], f["d"]
            if self.t % 4 == 0:         # a key frame: the tracked points gain observations, close stereo keypoints become map points
                tracked = mp[mp >= 0]
                tracked = tracked[~m.temporal[tracked]]
                np.add.at(m.obs, tracked, 2)
                has = (mp >= 0) & ~m.temporal[np.maximum(mp, 0)]
                cr = self._close_points_order(depth, has)
                if len(cr):
                    mp[cr] = self._new_points(k, d, depth, cr, Twc, 2, False)     # mvbOutlier is not touched (:1254-1265): a stale
                                                                                  # flag takes the new point from the frame below
            tmp = (mp >= 0) & m.temporal[np.maximum(mp, 0)]          # :578-596: the temporal points live for one frame
            mp[tmp] = -1
            outlier[tmp] = 0
            m.alive[m.temporal] = False
        mp[(mp >= 0) & (outlier != 0)] = -1                            # :606-610
        c["held"] = int((mp >= 0).sum())
        self._log("end", {}, dict(mp=mp.copy(), map_size=int(len(m.obs)), Tcw=Tcw.copy()))
        self.frames.append(c)
        return mp, Tcw, Twc

    def _keep(self, f, mp, Tcw, Twc, nf=None):
        self.last = {"k": np.array(f["k"]), "d": np.array(f["d"]), "uright": np.array(f["uright"]), "depth": np.array(f["depth"]), "mp": mp,
                     "Tcw": Tcw, "Twc": Twc, "frame": f, "nf": nf}
        self.poses.append(Tcw.copy())
        self.t += 1

    # ---------------------------------------------------------------------------------------------------- stereo
    def step_stereo(self, left, right, Tcw0=None):
        f = self.be.frame_stereo(left, right)
        k, d, depth = f["k"], f["d"], f["depth"]
        self._log("frame", {}, dict(k=np.array(k), d=np.array(d), uright=np.array(f["uright"]), depth=np.array(depth)))
        if self.t == 0:
            Tcw = np.ascontiguousarray(Tcw0, np.float32)
            Twc = twc_of(Tcw)
            mp = np.full(len(k), -1, np.int64)
            idx = np.nonzero(depth > 0)[0]
            mp[idx] = self._new_points(k, d, depth, idx, Twc, 2, False)
            self._log("end", {}, dict(mp=mp.copy(), map_size=int(len(self.map.obs)), Tcw=Tcw.copy()))
        else:
            mp, Tcw, Twc = self._track(f)
        self._keep(f, mp, Tcw, Twc)

    # ---------------------------------------------------------------------------------------------------- monocular
    def initialize_mono(self, img0, img1, nf):
        """MonocularInitialization on two frames + CreateInitialMapMonocular -> dict of what was decided"""
        be, m = self.be, self.map
        f0 = be.frame_mono(img0, nf)
        self._log("frame", {}, dict(k=np.array(f0["k"]), d=np.array(f0["d"])))
        self.t = 1
        f1 = be.frame_mono(img1, nf)
        self._log("frame", {}, dict(k=np.array(f1["k"]), d=np.array(f1["d"])))
        k0, k1 = np.array(f0["k"]), np.array(f1["k"])
        r = self.init = dict(ok=False, n0=len(k0), n1=len(k1))
        assert len(k0) > 100 and len(k1) > 100                               # :712, :733
        prev = np.stack([k0["x"], k0["y"]], 1).astype(np.float32)            # :716-718
        nm, m12, prev2 = be.search_init(f0, f1, prev, 100)
        self._log("search_init", dict(prev=prev), dict(n=nm, match=m12, prev=prev2))
        r["matches"] = int(nm)
        if nm < 100:                                                         # :746
            r["why"] = "matches < 100"
            return r
        i1 = np.nonzero(m12 >= 0)[0]
        matches = np.stack([i1, m12[i1]], 1).astype(np.int32)                 # mvMatches12 (src/Initializer.cc:55-69)
        sets = init_sets(self.seed, len(matches))
        ok, R21, t21, P3D, tri, info = be.initialize(f0, f1, matches, sets)
        self._log("initialize", dict(keys1=prev.copy(), keys2=np.stack([k1["x"], k1["y"]], 1).astype(np.float32), matches=matches, sets=sets),
                  dict(ok=ok, R21=R21, t21=t21, P3D=P3D, triangulated=tri, info=info))
        if not ok:
            r["why"] = "Initialize refused"
            return r
        keep = np.asarray(tri, bool)                                          # :759-766
        matches, P3D = matches[keep], np.asarray(P3D, np.float32)[keep]
        r["triangulated"] = int(keep.sum())
        Tcw1 = np.eye(4, dtype=np.float32)
        Tcw1[:3, :3], Tcw1[:3, 3] = R21, t21
        # CreateInitialMapMonocular
        desc2 = np.stack([np.array(f0["d"])[matches[:, 0]], np.array(f1["d"])[matches[:, 1]]], 1).reshape(-1, 32)
        off = (2 * np.arange(len(matches) + 1)).astype(np.int32)
        row = be.distinctive(desc2, off)
        self._log("distinctive", dict(desc=desc2, offsets=off), dict(row=np.asarray(row, np.int32)))
        desc = desc2[off[:-1] + np.asarray(row, np.int64)]
        ow0, ow1 = np.zeros(3, np.float32), twc_of(Tcw1)[:3, 3]
        u0, _, _ = self._ranges(P3D, ow0, k0["octave"][matches[:, 0]])
        u1, maxd, mind = self._ranges(P3D, ow1, k1["octave"][matches[:, 1]])   # mpRefKF = pKFcur
        normal = (((u0 + u1).astype(np.float32)) / np.float32(2)).astype(np.float32)
        ids = m.add(P3D, desc, normal, maxd, mind, 2, False)
        z = np.sort(P3D[:, 2].astype(np.float32))                            # the first key frame sits at the identity
        median = np.float32(z[(len(z) - 1) // 2])
        r["median_depth"], r["tracked"] = float(median), int(len(ids))
        if median < 0 or len(ids) < 100:                                      # :835
            r["why"] = "wrong initialisation"
            return r
        inv = np.float32(1.0) / median
        Tcw1[:3, 3] = (Tcw1[:3, 3] * inv).astype(np.float32)                  # :843-845
        m.pos = (m.pos * inv).astype(np.float32)                             # :848-856: the position only
        mp1 = np.full(len(k1), -1, np.int64)
        mp1[matches[:, 1]] = ids
        self._log("initial_map", {}, dict(pos=m.pos.copy(), desc=m.desc.copy(), normal=m.normal.copy(), maxd=m.maxd.copy(), mind=m.mind.copy(),
                                          Tcw=Tcw1.copy(), mp=mp1.copy()))
        self.kf = dict(ow0=ow0, ow1=twc_of(Tcw1)[:3, 3], lvl0=k0["octave"][matches[:, 0]], lvl1=k1["octave"][matches[:, 1]], ids=ids)
        self.poses = [np.eye(4, dtype=np.float32)]
        self.vel = Tcw1.copy()                       # the stated deviation: mCurrentFrame.mTcw * (the first frame's Twc = I)
        self._keep(f1, mp1, Tcw1, twc_of(Tcw1), nf=nf)
        r["ok"] = True
        return r

    def recompute_ranges(self):
        """MapPoint::UpdateNormalAndDepth for every initial point at its scaled position and the scaled key-frame centres: what
        LocalMapping does for a point once a key frame adds an observation of it.  NOT in the reference's tracking thread: a stated
        step of the monocular scene, after which isInFrustum accepts the initial points."""
        m, kf = self.map, self.kf
        u0, _, _ = self._ranges(m.pos[kf["ids"]], kf["ow0"], kf["lvl0"])
        u1, maxd, mind = self._ranges(m.pos[kf["ids"]], kf["ow1"], kf["lvl1"])
        m.normal[kf["ids"]] = (((u0 + u1).astype(np.float32)) / np.float32(2)).astype(np.float32)
        m.maxd[kf["ids"]], m.mind[kf["ids"]] = maxd, mind
        self._log("recompute_ranges", {}, dict(normal=m.normal.copy(), maxd=m.maxd.copy(), mind=m.mind.copy()))

    def step_mono(self, img, nf):
        f = self.be.frame_mono(img, nf)
        self._log("frame", {}, dict(k=np.array(f["k"]), d=np.array(f["d"])))
        mp, Tcw, Twc = self._track(f)
        self._keep(f, mp, Tcw, Twc, nf=nf)


def run_stereo(backend, frames, Tcw0, mutate=None, save_at=None):
    """-> the chain; .lost = the Lost that ended it or None; .saved = state() before frame save_at"""
    ch = Chain(backend, "stereo", mutate=mutate)
    ch.lost = ch.saved = None
    try:
        for t, (l, r) in enumerate(frames):
            if t == save_at:
                ch.saved = ch.state()
            ch.step_stereo(l, r, Tcw0 if t == 0 else None)
    except Lost as e:
        ch.lost = e
    return ch


def run_mono(backend, images, seed, nf_init, nf_track, mutate=None, recompute_at=None):
    """recompute_at: the frame before which recompute_ranges() is called"""
    ch = Chain(backend, "mono", seed=seed, mutate=mutate)
    ch.lost = None
    try:
        if ch.initialize_mono(images[0], images[1], nf_init)["ok"]:
            for t, img in enumerate(images[2:], 2):
                if t == recompute_at:
                    ch.recompute_ranges()
                ch.step_mono(img, nf_track)
    except Lost as e:
        ch.lost = e
    return ch


# ---------------------------------------------------------------------------------------------------- restatements, memoised
_memo = {}


def memo(stage, key, fn):
    """the restatements' results by input bytes: a stage is restated once per distinct input, whichever chain asks"""
    k = (stage, key)
    if k not in _memo:
        _memo[k] = fn()
    return _memo[k]


def restated_optimize(obs, Tcw, outlier):
    import pose_ref
    key = (obs.tobytes(), np.asarray(Tcw, np.float32).tobytes(), np.asarray(outlier, np.uint8).tobytes())
    return memo("optimize", key, lambda: pose_ref.pose_optimization(obs, CAM, Tcw, outlier=outlier))


def restated_initialize(keys1, keys2, matches, sets):
    import init_ref
    key = (keys1.tobytes(), keys2.tobytes(), matches.tobytes(), sets.tobytes())
    return memo("initialize", key, lambda: init_ref.initialize(keys1, keys2, matches, sets, K4, 1.0, 1.0, 50))


# ---------------------------------------------------------------------------------------------------- backends
class CpuBackend(TC.OracleBackend):
    """the restatements: the C oracle's extractor and matchers, init_ref, pose_ref"""
    name = "cpu"

    def __init__(self, w, h, nf):
        super().__init__(w, h, nf)
        self.sf = self.o.Extractor(nf, SCALE, NLEVELS, 20, 7).scale_factors

    def frame_stereo(self, left, right):
        return self.frame(left, right, BF, CAM[5])

    def frame_mono(self, img, nf):
        o = self.o
        ex = o.Extractor(nf, SCALE, NLEVELS, 20, 7)
        k, d = ex.extract(img)
        self.sf = ex.scale_factors
        return {"k": k, "d": d, "uright": np.full(len(k), -1.0, np.float32), "depth": np.full(len(k), -1.0, np.float32)}

    def search_frame(self, f, flast, Tc, Tl, lp, cur_mp, th, mono):
        return self.o.search_by_projection_frame(f["k"], f["d"], f["uright"], self.geom, self.sf, self.cam, Tc, Tl, lp, flast["d"],
                                                 cur_mp, None, th, mono, True)

    def optimize(self, f, obs, is2, Tcw, outlier):
        r = restated_optimize(obs, Tcw, outlier)
        return r["Tcw"].copy(), r["outlier"].copy(), r["ngood"], r

    def search_init(self, f0, f1, prev, window):
        return self.o.search_for_initialization(f0["k"], f0["d"], f1["k"], f1["d"], self.geom, prev, window, 0.9, True)

    def initialize(self, f0, f1, matches, sets):
        k1 = np.stack([f0["k"]["x"], f0["k"]["y"]], 1).astype(np.float32)
        k2 = np.stack([f1["k"]["x"], f1["k"]["y"]], 1).astype(np.float32)
        r = restated_initialize(k1, k2, matches, sets)
        return bool(r["result"]), r["R21"].copy(), r["t21"].copy(), r["P3D"].copy(), r["triangulated"].copy(), r

    def distinctive(self, desc, off):
        return np.array([self.o.distinctive_descriptor(desc[off[i]:off[i + 1]])[0] for i in range(len(off) - 1)], np.int32)


class GpuHostBackend(TC.GpuHostBackend):
    """the library through its host-array entry points"""
    name = "gpu-host"

    def __init__(self, w, h, nf):
        super().__init__(w, h, nf)
        self.mono_ex = {}

    def frame_stereo(self, left, right):
        return self.frame(left, right, BF, CAM[5])

    def _mono_ex(self, nf):
        if nf not in self.mono_ex:
            self.mono_ex[nf] = self.pkg.ORBextractor(nf, SCALE, NLEVELS, 20, 7)
        return self.mono_ex[nf]

    def frame_mono(self, img, nf):
        k, d = self._mono_ex(nf)(img)
        return {"k": k, "d": d, "uright": np.full(len(k), -1.0, np.float32), "depth": np.full(len(k), -1.0, np.float32)}

    def search_frame(self, f, flast, Tc, Tl, lp, cur_mp, th, mono):
        return self.matcher.SearchByProjectionFrame(f["k"], f["d"], f["uright"], self.geom, self.sf, self.cam, Tc, Tl, lp, flast["d"],
                                                    cur_mp, None, th, mono)

    def optimize(self, f, obs, is2, Tcw, outlier):
        return self.pkg.pose_optimization(obs, self.cam, Tcw, outlier)

    def search_init(self, f0, f1, prev, window):
        return self.matcher.SearchForInitialization(f0["k"], f0["d"], f1["k"], f1["d"], self.geom, prev, window)

    def initialize(self, f0, f1, matches, sets):
        k1 = np.stack([f0["k"]["x"], f0["k"]["y"]], 1).astype(np.float32)
        k2 = np.stack([f1["k"]["x"], f1["k"]["y"]], 1).astype(np.float32)
        ini = self.pkg.Initializer(k1, K4, sigma=1.0, iterations=len(sets))
        ok, R, t, P, tri, info = ini.initialize(k2, matches, sets, 1.0, 50)
        info = dict(info, search_call=ini.search(k2, matches, sets))               # FindHomography / FindFundamental alone, for the stage's rule
        return ok, R, t, P, tri, info

    def distinctive(self, desc, off):
        return self.pkg.distinctive_descriptors(desc, off)[0]


class GpuDeviceBackend(GpuHostBackend):
    """the frame stays in HBM.  Stereo: one orbx_stereo_frame_view call per frame, its record read there by the *_device matchers
    and by pose_optimization_device (d_kl, d_uright).  Monocular: extract_batch_device into tensors of this backend (two sets per
    extractor alternate: the last frame's stay valid), mvuRight = -1 in HBM; the device forms of SearchByProjection(cur, last),
    SearchLocalPoints, PoseOptimization and Initialize read them; SearchForInitialization and ComputeDistinctiveDescriptors have
    host-array entry points only."""
    name = "gpu-device"

    def __init__(self, w, h, nf):
        super().__init__(w, h, nf)
        import torch
        self.torch = torch
        self.ex = self.exl
        self.stream = torch.cuda.current_stream().cuda_stream
        self.sets = {}
        self.thr = self.pkg.predict_scale_thresholds(float(np.log(np.float32(SCALE)).astype(np.float32)), NLEVELS)

    def frame_stereo(self, left, right):
        f = self.ex.stereo_frame_view(left, right, BF, CAM[5])
        v = f["view"]
        return {"k": f["kl"], "d": f["dl"], "uright": f["uright"], "depth": f["depth"], "n": len(f["kl"]),
                "d_k": v.d_kl, "d_d": v.d_dl, "d_ur": v.d_uright, "keep": v}

    def frame_mono(self, img, nf):
        torch, ex = self.torch, self._mono_ex(nf)
        if nf not in self.sets:
            ex(np.zeros((self.h, self.w), np.uint8) + 90)               # plan
            cap = ex.max_keypoints()
            self.sets[nf] = dict(i=0, cap=cap, img=torch.zeros((1, self.h, self.w), dtype=torch.uint8, device="cuda"), s=[
                dict(kps=torch.zeros((1, cap, 7), dtype=torch.float32, device="cuda"), desc=torch.zeros((1, cap, 32), dtype=torch.uint8, device="cuda"),
                     cnt=torch.zeros(1, dtype=torch.int32, device="cuda"), ur=torch.full((cap,), -1.0, dtype=torch.float32, device="cuda"))
                for _ in range(2)])
        S = self.sets[nf]
        s = S["s"][S["i"] & 1]
        S["i"] += 1
        S["img"][0].copy_(torch.from_numpy(np.ascontiguousarray(img)))
        w, h, cap = self.w, self.h, S["cap"]
        ex.extract_batch_device(S["img"].data_ptr(), 1, w, h, w, w * h, s["kps"].data_ptr(), s["desc"].data_ptr(), s["cnt"].data_ptr(), cap, self.stream)
        torch.cuda.current_stream().synchronize()
        n = int(s["cnt"].cpu()[0])
        k = np.frombuffer(s["kps"][0, :n].cpu().numpy().tobytes(), self.pkg.KP_DTYPE)
        return {"k": k, "d": s["desc"][0, :n].cpu().numpy().copy(), "uright": np.full(n, -1.0, np.float32), "depth": np.full(n, -1.0, np.float32),
                "n": n, "d_k": s["kps"].data_ptr(), "d_d": s["desc"].data_ptr(), "d_ur": s["ur"].data_ptr(), "keep": s}

    def search_frame(self, f, flast, Tc, Tl, lp, cur_mp, th, mono):
        return self.pkg.search_by_projection_frame_device(f["d_k"], f["d_d"], f["d_ur"], f["n"], self.geom, self.sf, self.cam, Tc, Tl, lp,
                                                          flast["d_d"], cur_mp, None, th, mono, True, 0, self.stream)

    def search_local(self, f, wp, mp_desc, Tcw, frame_mp, ext_obs, th, nnratio, log_sf):
        return self.pkg.search_local_points_device(f["d_k"], f["d_d"], f["d_ur"], f["n"], self.geom, self.sf, wp, mp_desc, Tcw, self.cam,
                                                   0.5, self.thr, frame_mp, ext_obs, th, nnratio, 0, self.stream)

    def optimize(self, f, obs, is2, Tcw, outlier):
        pts = np.zeros(len(obs), self.pkg.POSE_WORLDPOS_DTYPE)
        for a in ("valid", "wx", "wy", "wz"):
            pts[a] = obs[a]
        return self.pkg.pose_optimization_device(f["d_k"], f["d_ur"], f["n"], is2, pts, self.cam, Tcw, outlier=outlier, stream=self.stream)

    def initialize(self, f0, f1, matches, sets):
        return self.pkg.initialize_device(f0["d_k"], f0["n"], f1["d_k"], f1["n"], matches, sets, K4, 1.0, 1.0, 50, stream=self.stream)


# ---------------------------------------------------------------------------------------------------- comparing traces
def entry_bytes(e):
    """a trace entry's outputs as bytes (the solvers' info is compared by the stage rules, not here)"""
    parts = [repr((e["stage"], e["frame"])).encode()]
    for k in sorted(e["out"]):
        v = e["out"][k]
        if k == "info":
            continue
        parts.append(k.encode() + (np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode()))
    return b"|".join(parts)


def digest(chain, first=0):
    return [entry_bytes(e) for e in chain.trace if e["frame"] >= first]


DEVICE_STAGES = ("frame", "project", "local", "optimize_motion", "optimize_local", "search_init", "initialize", "distinctive")


def first_difference(a, b, common=False, stages=None):
    """None if two chains left the same trace, else (frame, stage) of the first entry that differs (common: one chain may have
    stopped earlier; stages: only entries of these stages are compared, e.g. DEVICE_STAGES: what a backend produced, not what
    the bookkeeping logged of itself)"""
    for x, y in zip(a.trace, b.trace):
        if stages is not None and x["stage"] not in stages and x["stage"] == y["stage"]:
            continue
        if entry_bytes(x) != entry_bytes(y):
            return x["frame"], x["stage"]
    if len(a.trace) != len(b.trace) and not common:
        longer = a.trace if len(a.trace) > len(b.trace) else b.trace
        e = longer[min(len(a.trace), len(b.trace))]
        return e["frame"], e["stage"]
    return None
